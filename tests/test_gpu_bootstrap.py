"""GPU tests of the bootstrap mode (met2_fit_bootstrap, Met2Plan.fit_bootstrap, recon_met2_arrays(bootstrap=...)): the device's replicates
against the numpy restatement, the sigma estimate, the fused statistics against replicates + plan.fit + numpy, bit-identical point outputs,
invariance to call splitting, voxel order and chunking, what the spread means, gating, and the drivers."""
import importlib

import numpy as np
import pytest
import torch

from conftest import relmax_rows
from test_bootstrap_host import replicates_np

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def synth():
    return importlib.import_module(PKG + ".synth")


def make_plan(pkg, synth, nte=32, nt2=60, penalty="L2"):
    T2s = synth.t2_grid(nt2)
    plan = pkg.Met2Plan(nte, nt2, 1, device=0)
    plan.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, np.array([150.0]), 3000.0)
    return plan.set_penalty(penalty, T2s)


def composed_values(plan, method, out, n_rep, seed, vid=None):
    """replicates (met2_bootstrap_replicates) -> plan.fit -> [7, nvox, n_rep] values and [nvox, n_rep] status"""
    nvox = out["sig"].shape[0]
    reps = plan.bootstrap_replicates(out["sig"], out["sigma"], n_rep, seed, voxel_id=vid)
    fitted = (out["status"] & 1) != 0
    fr = plan.fit(method, reps.reshape(nvox * n_rep, plan.n_te), mask=fitted.repeat_interleave(n_rep))
    vals = torch.cat([fr["maps"], fr["reg"][None]], 0).reshape(7, nvox, n_rep).cpu().numpy()
    return vals, fr["status"].reshape(nvox, n_rep).cpu().numpy(), fitted.cpu().numpy()


def numpy_stats(vals):
    """[7, nvox, n_rep] -> [7, 5, nvox]: mean, std (ddof 1), np.quantile at 0.025, 0.5, 0.975"""
    q = np.quantile(vals, [0.025, 0.5, 0.975], axis=-1)                  # [3, 7, nvox]
    return np.concatenate([vals.mean(-1)[:, None], vals.std(-1, ddof=1)[:, None], np.moveaxis(q, 0, 1)], axis=1)


def test_generator_matches_numpy(pkg, synth):
    plan = make_plan(pkg, synth)
    data, _, _ = synth.make_voxels(4096, nte=32, seed=11, device="cuda:0")
    sigma = data[:, 0] / 100.0
    vid = (2 ** 32 + 12345 + 7919 * np.arange(4096)).astype(np.int64)
    c, s = data.cpu().numpy(), sigma.cpu().numpy()
    for seed in (0, -1):
        got = plan.bootstrap_replicates(data, sigma, 16, seed, voxel_id=torch.as_tensor(vid, device="cuda:0")).cpu().numpy()
        want = replicates_np(c, s, vid, 16, seed)
        assert relmax_rows(got.reshape(-1, 32), want.reshape(-1, 32)).max() <= 1e-13
    g0 = plan.bootstrap_replicates(data, sigma, 16, 0).cpu().numpy()         # voxel_id NULL = the voxel's index
    assert np.array_equal(g0, plan.bootstrap_replicates(data, sigma, 16, 0, voxel_id=torch.arange(4096, device="cuda:0")).cpu().numpy())
    z = plan.bootstrap_replicates(data, torch.zeros_like(sigma), 16, 5).cpu().numpy()
    assert np.array_equal(z, np.broadcast_to(c[:, None, :], z.shape))
    plan.close()


def test_sigma_estimate_and_given_sigma(pkg, synth):
    plan = make_plan(pkg, synth)
    data, _, _ = synth.make_voxels(1024, nte=32, seed=12, device="cuda:0")
    out = plan.fit_bootstrap("X2", data, n_rep=4, seed=1)
    nn = plan.fit("NNLS", data)
    M, f0, s0 = data.cpu().numpy(), nn["fsol"].cpu().numpy(), nn["sig"].cpu().numpy()
    want = np.sqrt(np.sum((M - s0) ** 2, axis=1) / np.maximum(32 - np.count_nonzero(f0 > 0, axis=1), 1))
    got = out["sigma"].cpu().numpy()
    assert np.max(np.abs(got - want) / want) <= 1e-12
    given = torch.linspace(0.5, 3.0, 1024, dtype=torch.float64, device="cuda:0")
    out2 = plan.fit_bootstrap("X2", data, n_rep=4, seed=1, sigma=given)
    assert torch.equal(out2["sigma"], given)
    plan.close()


CONFIGS = [("NNLS", "I", 32, 60), ("X2", "L2", 32, 60), ("L_curve", "L1", 32, 60), ("GCV", "L2", 32, 60), ("BayesReg", "InvT2", 32, 60),
           ("T2SPARC", "InvT2", 32, 96), ("X2", "L2", 48, 120)]


@pytest.mark.parametrize("method,penalty,nte,nt2", CONFIGS)
def test_fused_equals_composed_and_point_outputs(pkg, synth, method, penalty, nte, nt2):
    plan = make_plan(pkg, synth, nte, nt2, penalty)
    data, _, _ = synth.make_voxels(512, nte=nte, seed=13, device="cuda:0")
    B, seed = 32, 77
    out = plan.fit_bootstrap(method, data, n_rep=B, seed=seed, want_lambda=True)
    ref = plan.fit(method, data, want_lambda=True)
    for k in ("fsol", "sig", "reg", "lam", "maps", "status"):
        assert torch.equal(out[k], ref[k]), k
    vals, st, fitted = composed_values(plan, method, out, B, seed)
    assert fitted.all()
    want = numpy_stats(vals)
    got = out["stats"].cpu().numpy()
    assert np.array_equal(got[:, 2:], want[:, 2:])                          # quantiles bit-equal to np.quantile
    scale = np.abs(vals).max(-1)                                             # [7, nvox]
    assert np.all(np.abs(got[:, 0] - want[:, 0]) <= 1e-14 * scale)
    assert np.all(np.abs(got[:, 1] - want[:, 1]) <= 1e-12 * want[:, 1] + 1e-14 * scale)
    assert np.array_equal(out["rep_status"].cpu().numpy(), np.bitwise_or.reduce(st, axis=1))
    plan.close()


def test_invariance_to_splitting_and_order(pkg, synth):
    plan = make_plan(pkg, synth)
    data, _, _ = synth.make_voxels(3000, nte=32, seed=14, device="cuda:0")
    B, seed = 24, 2 ** 40 + 3
    one = plan.fit_bootstrap("X2", data, n_rep=B, seed=seed)
    cuts = [0, 1000, 1001, 3000]
    parts = [plan.fit_bootstrap("X2", data[a:b].contiguous(), n_rep=B, seed=seed, voxel_id=np.arange(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    for k in ("stats", "sigma", "rep_status"):
        assert torch.equal(one[k], torch.cat([p[k] for p in parts], dim=-1)), k
    perm = torch.as_tensor(np.random.default_rng(3).permutation(3000), device="cuda:0")
    pm = plan.fit_bootstrap("X2", data[perm].contiguous(), n_rep=B, seed=seed, voxel_id=perm)
    for k in ("stats", "sigma", "rep_status"):
        assert torch.equal(one[k][..., perm], pm[k]), k
    plan.close()


def test_lcurve_two_bins_per_lane_chunks_are_deterministic(pkg, synth):
    # 8 192 voxels x 16 replicates at 48 x 120: 32 internal fits of 4 096 rows through the spill-over kernel
    plan = make_plan(pkg, synth, 48, 120, "L1")
    data, _, _ = synth.make_voxels(8192, nte=48, seed=15, device="cuda:0")
    a = plan.fit_bootstrap("L_curve", data, n_rep=16, seed=9)
    b = plan.fit_bootstrap("L_curve", data, n_rep=16, seed=9)
    h = plan.fit_bootstrap("L_curve", data[4096:].contiguous(), n_rep=16, seed=9, voxel_id=np.arange(4096, 8192))
    for k in ("stats", "sigma", "rep_status"):
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k][..., 4096:], h[k]), k
    plan.close()


def test_bootstrap_spread_means_noise_propagation(pkg, synth):
    plan = make_plan(pkg, synth)
    n, snr, R = 2048, 100.0, 64
    clean, _, _ = synth.make_voxels(n, nte=32, seed=16, snr=(1e15, 1e15), device="cuda:0")     # noise-free to ~1e-15
    sg = clean[:, :1] / snr
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(5)
    draws = [torch.sqrt((clean + sg * torch.randn(clean.shape, dtype=torch.float64, device="cuda:0", generator=gen)) ** 2 +
                        (sg * torch.randn(clean.shape, dtype=torch.float64, device="cuda:0", generator=gen)) ** 2) for _ in range(R)]
    mwf = torch.stack([plan.fit("X2", d, want_sig=False)["maps"][0] for d in draws]).cpu().numpy()     # [R, n]
    emp = mwf.std(0, ddof=1)
    out = plan.fit_bootstrap("X2", draws[0], n_rep=64, seed=21, sigma=sg[:, 0])
    boot = out["stats"][0, 1].cpu().numpy()
    ok = emp > 0
    ratio = np.median(boot[ok] / emp[ok])
    print("median bootstrap / empirical std(MWF) = %.3f" % ratio)
    assert 0.67 <= ratio <= 1.5
    z = plan.fit_bootstrap("X2", draws[0], n_rep=16, seed=21, sigma=torch.zeros(n, dtype=torch.float64, device="cuda:0"))["stats"].cpu().numpy()
    assert np.all(z[:, 1] == 0.0)
    assert np.array_equal(z[:, 2], z[:, 3]) and np.array_equal(z[:, 3], z[:, 4])
    assert np.array_equal(z[:, 0], z[:, 3])
    plan.close()


def test_gated_voxels_get_zero_stats(pkg, synth):
    plan = make_plan(pkg, synth)
    data, _, _ = synth.make_voxels(256, nte=32, seed=17, device="cuda:0")
    data[1] = 0.0
    data[2, 5] = float("nan")
    mask = torch.ones(256, dtype=torch.uint8, device="cuda:0")
    mask[0] = 0
    out = plan.fit_bootstrap("X2", data, n_rep=8, seed=4, mask=mask)
    ref = plan.fit("X2", data, mask=mask)
    assert torch.equal(out["status"], ref["status"])
    for k in ("fsol", "reg", "maps"):
        assert torch.equal(out[k], ref[k]), k
    st = out["stats"].cpu().numpy()
    assert np.all(st[:, :, :3] == 0.0) and np.all(out["rep_status"][:3].cpu().numpy() == 0)
    assert np.all(st[5, 1, 3:] > 0.0) and np.all((out["rep_status"][3:].cpu().numpy() & 1) == 1)       # TWC spreads wherever noise is drawn
    plan.close()


def test_volume_layouts(pkg, synth):
    plan = make_plan(pkg, synth)
    data, _, _ = synth.make_voxels(6 * 5 * 4, nte=32, seed=18, device="cuda:0")
    vol = data.reshape(6, 5, 4, 32)
    fvol = vol.permute(3, 2, 1, 0).contiguous().permute(3, 2, 1, 0)            # Fortran order, as nibabel's arrays
    vid = np.arange(120).reshape(6, 5, 4)
    c = plan.fit_bootstrap("X2", vol, n_rep=8, seed=6, voxel_id=vid)
    f = plan.fit_bootstrap("X2", fvol, n_rep=8, seed=6, voxel_id=vid)
    assert c["stats"].shape == (7, 5, 6, 5, 4) and c["sigma"].shape == (6, 5, 4)
    for k in ("stats", "sigma", "rep_status", "maps"):
        assert torch.equal(c[k], f[k]), k
    plan.close()


def test_driver_bootstrap(pkg, synth, tmp_path):
    motor = importlib.import_module(PKG + ".motor")
    nifti = importlib.import_module(PKG + ".nifti")
    data, mask = synth.make_phantom((10, 9, 6), nte=32, seed=19)
    d, m = data.cpu().numpy(), mask.cpu().numpy()
    TE = 10.0 * np.arange(1, 33)
    names = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param")
    plain = motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    boot = motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", "brute-force", 40.0, bootstrap=dict(n_rep=8, seed=2))
    for k in names:
        assert np.array_equal(plain[k], boot[k]), k
    assert "data_prepared" not in boot
    for q in pkg.BOOT_QUANTITIES:
        assert boot[q + "_bootstrap"].shape == (10, 9, 6, 5)
    inside = m > 0
    assert np.all(boot["MWF_bootstrap"][~inside] == 0.0)
    assert np.all(boot["TWC_bootstrap"][inside & (boot["reg_param"] > 0)][:, 1] > 0.0)
    # the caller's own plan: the same statistics (voxel_id is the C-order flat index either way)
    mine = motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", "brute-force", 40.0, devices=None, plan=_driver_plan(pkg, TE),
                                   bootstrap=dict(n_rep=8, seed=2))
    for q in pkg.BOOT_QUANTITIES:
        assert np.array_equal(mine[q + "_bootstrap"], boot[q + "_bootstrap"]), q
    aff = np.diag([1.5, 1.5, 3.0, 1.0])
    nifti.save(nifti.NiftiImage(np.asfortranarray(d), aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(m.astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/recon_"
    res = motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None",
                                 "brute-force", "no", 40.0, bootstrap=dict(n_rep=8, seed=2))
    for q in pkg.BOOT_QUANTITIES:
        got = nifti.load(out + q + "_bootstrap.nii.gz").get_fdata()
        assert got.shape == (10, 9, 6, 5)
        assert np.array_equal(got, res[q + "_bootstrap"])
        assert np.array_equal(got, boot[q + "_bootstrap"])
    sg = nifti.load(out + "sigma.nii.gz").get_fdata()
    assert sg.shape == (10, 9, 6) and np.array_equal(sg, boot["sigma"])
    with pytest.raises(ValueError, match="bootstrap"):
        motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", "brute-force", 40.0, bootstrap=dict(n_rep=8, sed=2))


def _driver_plan(pkg, TE):
    import math
    T2s = np.logspace(math.log10(10.0), math.log10(2000.0), num=60, endpoint=True, base=10.0)
    plan = pkg.Met2Plan(32, 60, 91, device=0)
    plan.build_dictionary_epg(T2s, 1000.0 * np.ones(60), float(TE[1] - TE[0]), np.linspace(90.0, 180.0, 91), 3000.0)
    return plan.set_penalty("L2", T2s)
