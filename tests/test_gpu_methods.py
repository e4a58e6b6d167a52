"""GPU tests for the remaining §8(a) rows: BayesReg (BR), GCV (GC), brute-force FA (F1), the
objective functions on a lambda grid, the per-function drop-ins and the end-to-end driver mirror."""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, relmax, relmax_rows

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
TOL = 1e-5


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    from oracle import oracle
    oracle.build()
    return importlib.import_module(PKG)


def _single_fa_plan(pkg, g, pen):
    Dic = np.ascontiguousarray(g["Dic_full"][:, :, 60:61])
    plan = pkg.Met2Plan(int(g["nte"]), int(g["npc"]), 1)
    plan.set_dictionary(Dic).set_t2_grid(g["T2s"]).set_penalty(g["L_" + pen]).set_lambda_grid(g["lambda_grid"])
    return plan


@pytest.mark.parametrize("pen", ["I", "L1", "L2", "InvT2"])
def test_bayesreg_golden(pkg, gS1, pen):
    # BR (bayesian_interpolation.py:84-126) against the reference.  InvT2: flat evidence minimum: on the
    # 4 096-voxel fixture 7 % of voxels exceed 1e-5 (reference vs oracle: 6.5 %), all < 1.1e-4 (tests/test_tail_parity.py);
    # on these 32 voxels measured 0 over 1e-5, max 9.0e-6 -> at most 6 (3x the 7 % rate), all < 2e-4, MWF < 1e-5.
    import torch
    g = gS1
    plan = _single_fa_plan(pkg, g, pen)
    out = plan.fit("BayesReg", torch.as_tensor(g["data"], device="cuda"), want_lambda=True)
    f = out["fsol"].cpu().numpy() / g["data"][:, :1]
    e = relmax_rows(f, g["bayes_f_" + pen])
    lam = out["lam"].cpu().numpy()
    if pen == "L2":     # det(L2) = 0 -> objective +inf everywhere -> Brent's upper end point
        assert np.all(lam == 1.9999959949686712)
    print("MEASURED bayes_golden %s n_over=%d of %d max=%.2e" % (pen, int((e >= TOL).sum()), e.shape[0], e.max()))
    if pen == "InvT2":
        assert int((e >= TOL).sum()) <= 6 and e.max() < 2e-4, e
    else:
        assert e.max() < TOL, e
    T2s = g["T2s"]
    mwf = lambda x: x[:, T2s <= 40.0].sum(axis=1) / (x.sum(axis=1) + 1e-16)
    assert np.max(np.abs(mwf(f) - mwf(g["bayes_f_" + pen]))) < TOL


@pytest.mark.parametrize("meth,pen", [("X2", "L2"), ("BayesReg", "I"), ("BayesReg", "InvT2"), ("GCV", "I"), ("GCV", "L2")])
def test_objective_grid_golden(pkg, gS1, meth, pen):
    # objective functions on a fixed lambda grid (algorithms.py:226-233, :285-296 incl. the
    # diagonal-vector quirk; bayesian_interpolation.py:107-126) against the reference's values
    import torch
    from oracle import oracle
    g = gS1
    plan = _single_fa_plan(pkg, g, pen)
    lams = g["obj_grid"]
    data = torch.as_tensor(g["data"][:2], device="cuda")
    got = plan.objective_grid(meth, data, lams).cpu().numpy()
    if meth == "X2":
        M = g["data"][:2] / g["data"][:2, :1]
        ref = np.stack([oracle.objective("X2", g["D150"], M[v], g["L_" + pen], lams) for v in range(2)])
        assert np.allclose(got, ref, rtol=1e-9, atol=1e-12)
    elif meth == "BayesReg":
        ref = g["bayesobj_" + pen]
        well = lams >= 1e-1
        assert np.allclose(got[:, well], ref[:, well], rtol=1e-9, atol=1e-9)
        mid = lams >= 1e-4
        assert np.allclose(got[:, mid], ref[:, mid], rtol=1e-6, atol=1e-6)
    else:
        ref = g["gcvobj_" + pen]
        d = np.abs(got - ref)        # ~1e-5 (near-cutoff singular values) or ~0.1 (one rank step)
        assert np.median(d) < 1e-3 and np.max(d) < 0.3, (got, ref)


@pytest.mark.parametrize("pen", ["I", "L2"])
def test_gcv_distribution(pkg, gS1, pen):
    # GC: voxelwise parity is unattainable: accept on (i) the objective goldens above,
    # (ii) near-optimality of the device's lambda under the oracle's objective, (iii) MWF distribution.
    import torch
    from oracle import oracle
    g = gS1
    plan = _single_fa_plan(pkg, g, pen)
    out = plan.fit("GCV", torch.as_tensor(g["data"], device="cuda"), want_lambda=True)
    lam = out["lam"].cpu().numpy()
    f = out["fsol"].cpu().numpy() / g["data"][:, :1]
    M = g["data"] / g["data"][:, :1]
    T2s = g["T2s"]
    mwf = lambda x: x[T2s <= 40.0].sum() / (x.sum() + 1e-16)
    dm = []; do = []
    for v in range(g["data"].shape[0]):
        o2 = oracle.objective("GCV", g["D150"], M[v], g["L_" + pen], np.array([lam[v], g["gcv_lam_" + pen][v]]))
        do.append(o2[0] - o2[1])
        assert o2[0] <= o2[1] + 0.12, (v, o2)          # one step of the rank staircase is ~0.09 (measured max 8.9e-2)
        dm.append(abs(mwf(f[v]) - mwf(g["gcv_f_" + pen][v])))
    print("MEASURED gcv_dist %s dobj max=%.3e median=%.3e  dMWF median=%.2e max=%.2e" % (pen, max(do), np.median(do), np.median(dm), np.max(dm)))
    # measured: median |dMWF| 9.2e-8 (I) / 2.1e-7 (L2), max 6.2e-3 / 3.9e-5, median objective difference <= 0; the 4 096-voxel
    # distribution against the reference is in tests/test_tail_parity.py
    # (a single voxel can sit a rank step away: max 2.3e-2 here, 2.3e-2 among the 4 096 voxels of the tail fixture, whose bound is 7e-2)
    assert np.median(dm) < 1e-6 and np.max(dm) < 7e-2 and np.median(do) <= 1e-6, (dm, do)
    assert not (out["status"].cpu().numpy() & 32).any()


def test_fa_bruteforce_golden(pkg, gS1):
    # F1 (fa_estimation.py:74-90): argmin over 91 flip angles + km, against the reference
    import torch
    g = gS1
    plan = pkg.Met2Plan(int(g["nte"]), int(g["npc"]), 91)
    plan.set_dictionary(g["Dic_full"])
    data = torch.as_tensor(g["fa_data"], device="cuda")
    fa, km, resid = plan.fa_bruteforce(data, want_resid=True)
    assert np.array_equal(fa.cpu().numpy(), g["fa_idx"])
    assert np.allclose(km.cpu().numpy(), g["fa_km"], rtol=1e-7)
    # gating: masked-out and empty voxels
    d2 = data.clone(); d2[1] = 0.0
    mask = torch.ones(d2.shape[0], dtype=torch.uint8, device="cuda"); mask[0] = 0
    fa2, km2, _ = plan.fa_bruteforce(d2, mask)
    assert fa2[0] == 0 and km2[0] == 0 and fa2[1] == 0 and km2[1] == 0
    assert np.array_equal(fa2.cpu().numpy()[2:], g["fa_idx"][2:])


def test_fa_vs_oracle(pkg):
    import torch
    from oracle import oracle
    synth = importlib.import_module(PKG + ".synth")
    nte, nt2 = 32, 60
    T2s = synth.t2_grid(nt2); T1s = 1000.0 * np.ones(nt2); alphas = np.linspace(90.0, 180.0, 91)
    plan = pkg.Met2Plan(nte, nt2, 91)
    plan.build_dictionary_epg(T2s, T1s, 10.0, alphas, 3000.0)
    data, fa_true, _ = synth.make_voxels(300, nte=nte, seed=21, fa_values=alphas, device="cuda")
    fa, km, resid = plan.fa_bruteforce(data, want_resid=True)
    D = np.ascontiguousarray(np.transpose(plan.get_dictionary(), (2, 0, 1)))
    idx, kmo, sse, f, ro = oracle.fa_bruteforce(D, data.cpu().numpy(), np.ones(300), nthreads=8, want_resid=True)
    assert np.allclose(resid.cpu().numpy(), ro, rtol=1e-7, atol=1e-9)
    assert np.array_equal(fa.cpu().numpy(), idx)
    assert np.allclose(km.cpu().numpy(), kmo, rtol=1e-7)
    assert np.mean(np.abs(fa.cpu().numpy() - fa_true.cpu().numpy()) <= 3) > 0.8      # it does estimate the flip angle


def test_dropin_functions_golden(pkg, gS1):
    # per-function mirrors of intravoxel_algorithms / epg / fa_estimation / motor
    g = gS1
    ia = importlib.import_module(PKG + ".intravoxel_algorithms")
    epg = importlib.import_module(PKG + ".epg")
    faa = importlib.import_module(PKG + ".flip_angle_algorithms")
    motor = importlib.import_module(PKG + ".motor")
    D = g["D150"]; M = g["data"][0] / g["data"][0, 0]
    x, rn = ia.nnls(D, M)
    assert relmax(x, g["nnls_x"][0]) < TOL and abs(rn - g["nnls_rnorm"][0]) < 1e-7
    assert relmax(ia.nnls_tik(D, M, g["L_L2"], g["tik_lams"][2]), g["tik_L2"][2, 0]) < TOL
    f, lam, kest = ia.nnls_x2(D, M, g["L_L1"], 1.02)
    assert relmax(f, g["x2_f_L1"][0]) < TOL and abs(lam - g["x2_lam_L1"][0]) < 1e-6 * lam and abs(kest - g["x2_kest_L1"][0]) < 1e-6
    assert ia.nnls_lcurve_wrapper(D, M, g["L_I"], g["lambda_grid"]) == g["lc_lam_I"][0]
    f, lam = ia.BayesReg_nnls(D, M, g["L_I"])
    assert relmax(f, g["bayes_f_I"][0]) < TOL and abs(lam - g["bayes_lam_I"][0]) < 1e-6 * lam
    f, lam = ia.nnls_gcv(D, M, g["L_I"])
    assert f.shape == (60,) and 1e-8 <= lam <= 10.0
    with pytest.raises(ValueError):
        ia.nnls(D, np.full(32, np.nan))
    Dic = epg.create_Dic_3D(60, g["T2s"], g["T1s"], 32, 10.0, g["fa_sel"], 3000.0)
    assert relmax(Dic, g["Dic_sel"]) < 1e-12
    assert relmax(epg.create_met2_design_matrix_epg(60, g["T2s"], g["T1s"], 32, 10.0, 150.0, 3000.0), D) < 1e-12
    idx, alpha, km, sse, ff = faa.compute_optimal_FA(g["fa_data"][0], g["Dic_full"], g["alpha_values"])
    assert idx == int(g["fa_idx"][0]) and alpha == g["fa_alpha"][0] and abs(km - g["fa_km"][0]) < 1e-6 * km
    assert abs(sse - g["fa_sse"][0]) < 1e-6 * sse and relmax(ff, g["fa_f"][0]) < TOL
    for order, name in ((0, "I"), (1, "L1"), (2, "L2")):
        assert np.array_equal(motor.create_Laplacian_matrix(60, order), g["L_" + name])
    assert np.array_equal(motor.create_InvT2_matrix(g["T2s"]), g["L_InvT2"])
    fs, sg, rg = motor.fitting_slice_T2(g["row_mask"], g["row_data"], g["row_fa_index"], 12, g["Dic_full"], g["lambda_grid"], 60, 32,
                                        "X2", g["L_L2"], None)
    assert np.max(relmax_rows(fs, g["row_X2_L2_fsol"])) < TOL and np.allclose(rg, g["row_X2_L2_reg"], rtol=1e-4)


def test_driver_end_to_end_golden(pkg):
    # steps 2-4 of motor_recon_met2 (brute-force FA -> X2/L2 fit -> metrics) against the reference's own
    # run on a tiny in-memory volume (tests/golden/make_goldens.py: gen_motor)
    motor = importlib.import_module(PKG + ".motor")
    g = np.load(os.path.join(GOLDEN, "golden_motor_x2_l2_bf.npz"))
    res = motor.recon_met2_arrays(g["data"], g["mask"], g["TE"], 3000.0, "X2", "L2", "brute-force", 40.0)
    assert np.array_equal(res["FA"], g["FA"])
    assert relmax(res["fsol_4D"], g["fsol_4D"]) < TOL
    assert relmax(res["Est_Signal"], g["Est_Signal"]) < TOL
    assert np.allclose(res["reg_param"], g["reg_param"], rtol=1e-4, atol=1e-12)
    for name in ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC"):
        scale = max(1.0, np.max(np.abs(g[name])))
        assert np.max(np.abs(res[name] - g[name])) / scale < TOL, name


def test_spline_fa_and_driver_golden(pkg):
    # spline FA estimation (fa_estimation.py:35-70) + L-curve/L1 + metrics, against the
    # reference's own end-to-end run (spline is the CLI default, run_real_data_script.py:34)
    import torch
    from oracle import oracle
    motor = importlib.import_module(PKG + ".motor")
    faa = importlib.import_module(PKG + ".flip_angle_algorithms")
    g = np.load(os.path.join(GOLDEN, "golden_motor_lcurve_l1_spline.npz"))
    res = motor.recon_met2_arrays(g["data"], g["mask"], g["TE"], 3000.0, "L_curve", "L1", "spline", 40.0)
    assert np.array_equal(res["FA"], g["FA"])
    assert relmax(res["fsol_4D"], g["fsol_4D"]) < TOL
    assert np.array_equal(res["reg_param"], g["reg_param"])
    for name in ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC"):
        assert np.max(np.abs(res[name] - g[name])) / max(1.0, np.max(np.abs(g[name]))) < TOL, name
    # the per-row mirror against the oracle, including the continuous minimiser
    synth = importlib.import_module(PKG + ".synth")
    T2s = synth.t2_grid(60); T1s = 1000.0 * np.ones(60)
    ah = np.linspace(90.0, 180.0, 273); al = np.linspace(90.0, 180.0, 15)
    ph = pkg.Met2Plan(32, 60, 273); ph.build_dictionary_epg(T2s, T1s, 10.0, ah, 3000.0)
    pl = pkg.Met2Plan(32, 60, 15); pl.build_dictionary_epg(T2s, T1s, 10.0, al, 3000.0)
    data, fa_true, _ = synth.make_voxels(400, nte=32, seed=41, fa_values=ah, device="cuda")
    mask = torch.ones(400, dtype=torch.uint8, device="cuda"); mask[3] = 0
    fa, km, xmin = ph.fa_spline(pl, al, ah, data, mask, want_xmin=True)
    Dh = np.ascontiguousarray(np.transpose(ph.get_dictionary(), (2, 0, 1)))
    Dl = np.ascontiguousarray(np.transpose(pl.get_dictionary(), (2, 0, 1)))
    idx, kmo, xm = oracle.fa_spline(Dl, al, Dh, ah, data.cpu().numpy(), mask.cpu().numpy().astype(float), nthreads=8)
    assert np.allclose(xmin.cpu().numpy(), xm, rtol=1e-7, atol=1e-6)
    assert np.mean(fa.cpu().numpy() == idx) > 0.995 and np.max(np.abs(fa.cpu().numpy() - idx)) <= 1
    same = fa.cpu().numpy() == idx
    assert np.allclose(km.cpu().numpy()[same], kmo[same], rtol=1e-6)
    assert fa[3] == 0 and km[3] == 0
    assert np.mean(np.abs(ah[fa.cpu().numpy().astype(int)] - ah[fa_true.cpu().numpy().astype(int)]) <= 3.0) > 0.7      # it does estimate the flip angle


def test_file_level_driver_on_disk_contract(pkg, tmp_path):
    # NIfTI in, the driver's ten NIfTI volumes out (motor:167-182, 475-503)
    motor = importlib.import_module(PKG + ".motor")
    nifti = importlib.import_module(PKG + ".nifti")
    g = np.load(os.path.join(GOLDEN, "golden_motor_x2_l2_bf.npz"))
    aff = np.diag([1.5, 1.5, 3.0, 1.0])
    nifti.save(nifti.NiftiImage(g["data"], aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(g["mask"].astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/recon_"
    motor.motor_recon_met2(g["TE"], str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None",
                           "brute-force", "no", 40.0, 1)
    for name in ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param"):
        img = nifti.load(out + name + ".nii.gz")
        assert np.allclose(img.affine, aff)
        got = img.get_fdata()
        assert got.shape == g[name].shape
        if name == "FA":
            assert np.array_equal(got, g[name])
        elif name == "reg_param":
            assert np.allclose(got, g[name], rtol=1e-4, atol=1e-12)
        else:
            assert np.max(np.abs(got - g[name])) / max(1.0, np.max(np.abs(g[name]))) < TOL, name
    with pytest.raises(ValueError):
        motor.motor_recon_met2(g["TE"], str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "wavelet",
                               "brute-force", "no", 40.0, 1)
    # denoise='TV' (motor:293-304; parity unpinned, see tv.py): runs, writes Data_denoised.nii.gz like the reference, and the
    # denoised volume has a smaller total variation than the input
    res_tv = motor.motor_recon_met2(g["TE"], str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "TV",
                                    "brute-force", "no", 40.0, 1)
    den = nifti.load(out + "Data_denoised.nii.gz").get_fdata()
    src = g["data"] * g["mask"][..., None]
    tvn = lambda a: sum(np.abs(np.diff(a, axis=ax)).sum() for ax in range(3))
    assert den.shape == src.shape and np.isfinite(den).all() and tvn(den) < tvn(src)
    assert np.isfinite(res_tv["MWF"]).all()


def test_nesma_filter_and_driver_golden(pkg, tmp_path):
    # the NESMA filter (motor:305-333) -- bit-exact against the rows the reference's driver
    # produced, then the whole denoise='NESMA' run (brute-force FA, X2/L2, metrics) against the reference's maps
    motor = importlib.import_module(PKG + ".motor")
    nifti = importlib.import_module(PKG + ".nifti")
    g = np.load(os.path.join(GOLDEN, "golden_nesma.npz"))
    dm = g["data"] * g["mask"][..., None]
    dm = np.where(dm < 0, 0.0, dm)
    den = motor.nesma_filter(dm, g["mask"])
    assert np.array_equal(den, g["denoised"], equal_nan=True)
    res = motor.recon_met2_arrays(g["data"], g["mask"], g["TE"], 3000.0, "X2", "L2", "brute-force", 40.0, denoise="NESMA")
    assert np.array_equal(res["FA"], g["FA"])
    assert relmax(res["fsol_4D"], g["fsol_4D"]) < TOL
    assert np.allclose(res["reg_param"], g["reg_param"], rtol=1e-4, atol=1e-12)
    assert np.max(np.abs(res["MWF"] - g["MWF"])) < TOL
    # the on-disk driver with the same switch
    aff = np.eye(4)
    nifti.save(nifti.NiftiImage(g["data"], aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(g["mask"].astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/nesma_"
    motor.motor_recon_met2(g["TE"], str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "NESMA",
                           "brute-force", "no", 40.0, 1)
    assert np.max(np.abs(nifti.load(out + "MWF.nii.gz").get_fdata() - g["MWF"])) < TOL
    assert np.array_equal(nifti.load(out + "FA.nii.gz").get_fdata(), g["FA"])


def test_gaussian_smooth_and_default_pipeline_golden(pkg, tmp_path):
    # the CLI's default pipeline (spline FA on Gaussian-smoothed echoes, X2/L2 on the unsmoothed ones; motor:337-343):
    # the device filter is bit-identical to scipy.ndimage.gaussian_filter and to the rows the reference's driver used,
    # and the whole run reproduces the reference's maps
    import torch
    import scipy.ndimage as filt
    motor = importlib.import_module(PKG + ".motor")
    nifti = importlib.import_module(PKG + ".nifti")
    g = np.load(os.path.join(GOLDEN, "golden_motor_default_smooth.npz"))
    dm = g["data"] * g["mask"][..., None]
    dm = np.where(dm < 0, 0.0, dm)
    assert np.array_equal(motor.gaussian_smooth(dm, 2.0), g["smoothed"])
    rng = np.random.default_rng(8)
    for shp in [(33, 7, 20, 3), (1, 2, 3, 4), (12, 40, 5, 32)]:
        d = rng.standard_normal(shp)
        ref = np.stack([filt.gaussian_filter(d[..., c], 2.0, 0) for c in range(shp[-1])], axis=-1)
        got = motor.gaussian_smooth(torch.as_tensor(d, device="cuda"), 2.0)
        assert np.array_equal(got.cpu().numpy(), ref), shp
    res = motor.recon_met2_arrays(g["data"], g["mask"], g["TE"], 3000.0, "X2", "L2", "spline", 40.0, FA_smooth="yes")
    assert np.array_equal(res["FA"], g["FA"])
    assert relmax(res["fsol_4D"], g["fsol_4D"]) < TOL
    assert relmax(res["Est_Signal"], g["Est_Signal"]) < TOL
    assert np.allclose(res["reg_param"], g["reg_param"], rtol=1e-4, atol=1e-12)
    for name in ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC"):
        assert np.max(np.abs(res[name] - g[name])) / max(1.0, np.max(np.abs(g[name]))) < TOL, name
    # the same through the on-disk driver
    aff = np.eye(4)
    nifti.save(nifti.NiftiImage(g["data"], aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(g["mask"].astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/default_"
    motor.motor_recon_met2(g["TE"], str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None",
                           "spline", "yes", 40.0, 1)
    assert np.array_equal(nifti.load(out + "FA.nii.gz").get_fdata(), g["FA"])
    assert np.max(np.abs(nifti.load(out + "MWF.nii.gz").get_fdata() - g["MWF"])) < TOL
    with pytest.raises(pkg.Met2Error):
        motor.gaussian_smooth(np.zeros((2, 2, 2, 2)), sigma=9.0)        # radius 36 > 32


def test_roi_mode_x2(pkg):
    # ROI-mode fits (motor_recon_met2_real_data_ROI.py:405-443): mean signal, mean kernel, X2 with factor 1.01
    from oracle import oracle
    motor = importlib.import_module(PKG + ".motor")
    synth = importlib.import_module(PKG + ".synth")
    T2s = synth.t2_grid(60); T1s = 1000.0 * np.ones(60); alphas = np.linspace(90.0, 180.0, 91)
    Dic = importlib.import_module(PKG + ".epg").create_Dic_3D(60, T2s, T1s, 32, 10.0, alphas, 3000.0)
    data, fa, _ = synth.make_voxels(600, nte=32, seed=51, fa_values=alphas, device="cuda")
    data = data.cpu().numpy(); fa = fa.cpu().numpy()
    rng = np.random.default_rng(2)
    rois = rng.integers(0, 5, 600)                                  # label 0 = background
    L = motor.create_Laplacian_matrix(60, 2)
    res = motor.recon_met2_rois(data, rois, fa, Dic, T2s, L)
    assert list(res["labels"]) == [1, 2, 3, 4]
    for i, v in enumerate(res["labels"]):
        sel = rois == v
        tk = sum(Dic[:, :, int(k)] for k in fa[sel]) / sel.sum()
        ts = data[sel].sum(axis=0) / sel.sum()
        x, lam, kest = oracle.nnls_x2(tk, ts, L, 1.01)
        xs = x / (x.sum() + 1e-16)
        assert relmax(res["fsol"][i], xs) < TOL
        assert abs(res["reg_opt"][i] - lam) < 1e-5 * max(lam, 1e-3) and abs(res["k_est"][i] - kest) < 1e-6
        assert abs(res["MWF"][i] - xs[T2s <= 40.0].sum()) < TOL
