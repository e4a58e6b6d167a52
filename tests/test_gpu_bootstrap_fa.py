"""GPU tests of the bootstrap with the flip angle re-estimated per replicate and with spectrum bands (met2_fit_bootstrap_fa,
Met2Plan.fit_bootstrap(fa=..., want_spectrum=...), recon_met2_arrays(bootstrap=dict(fa=..., spectrum=...))): the fixed mode against the
older entry, the fused call against replicates + FA walk + plan.fit + numpy, invariance to splitting and order, gating, sigma 0, layouts
and drivers, and what the two modes of spread measure."""
import importlib
import os

import numpy as np
import pytest
import torch

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


class Plans:
    """A plan with the driver's FA axis (motor:231-244): 91 angles from 90 to 180 degrees for brute force; 273 and a coarse plan of 15
    attached for the spline method."""

    def __init__(self, pkg, synth, nte=32, nt2=60, penalty="L2", fa="brute-force", attach=True):
        T2s = synth.t2_grid(nt2)
        self.alphas = np.linspace(90.0, 180.0, 273 if fa == "spline" else 91)
        self.alpha_lr = np.linspace(90.0, 180.0, 15)
        self.plan = pkg.Met2Plan(nte, nt2, self.alphas.shape[0], device=0)
        self.plan.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, self.alphas, 3000.0).set_penalty(penalty, T2s)
        self.coarse = None
        if fa == "spline":
            self.coarse = pkg.Met2Plan(nte, nt2, 15, device=0)
            self.coarse.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, self.alpha_lr, 3000.0)
            if attach:
                self.plan.attach_fa_spline(self.coarse, self.alpha_lr)
        self.fa = fa

    def estimate(self, data, mask=None):
        """the FA index of every row, as the bootstrap's mode estimates it"""
        if self.fa == "spline":
            return self.plan.fa_spline(self.coarse, self.alpha_lr, self.alphas, data, mask, want_km=False)[0]
        return self.plan.fa_bruteforce(data, mask)[0]

    def close(self):
        self.plan.close()
        if self.coarse is not None:
            self.coarse.close()


def numpy_stats(vals):
    """[..., n_rep] -> [5, ...]: mean, std (ddof 1), np.quantile at 0.025, 0.5, 0.975"""
    q = np.quantile(vals, [0.025, 0.5, 0.975], axis=-1)
    return np.concatenate([vals.mean(-1)[None], vals.std(-1, ddof=1)[None], q], axis=0)


def check_stats(got, vals, what):
    """got [5, ...] against the numpy statistics of vals [..., n_rep], with the tolerances of test_fused_equals_composed_and_point_outputs"""
    want = numpy_stats(vals)
    scale = np.abs(vals).max(-1)
    dm = np.abs(got[0] - want[0])
    ds = np.abs(got[1] - want[1])
    print("%s: max |mean diff| / scale = %.3g, max |std diff| / (std + scale) = %.3g, quantiles equal = %s"
          % (what, np.max(dm / np.maximum(scale, 1e-300)), np.max(ds / np.maximum(want[1] + scale, 1e-300)), np.array_equal(got[2:], want[2:])))
    assert np.array_equal(got[2:], want[2:]), what                            # quantiles bit-equal to np.quantile
    assert np.all(dm <= 1e-14 * scale), what
    assert np.all(ds <= 1e-12 * want[1] + 1e-14 * scale), what


def test_fixed_mode_is_the_old_entry(pkg, synth):
    P = Plans(pkg, synth)
    data, fa_true, _ = synth.make_voxels(512, nte=32, seed=31, fa_values=P.alphas, device="cuda:0")
    old = P.plan.fit_bootstrap("X2", data, n_rep=32, seed=77, fa_index=fa_true, want_lambda=True)
    new = P.plan.fit_bootstrap("X2", data, n_rep=32, seed=77, fa_index=fa_true, want_lambda=True, fa="fixed", want_spectrum=True)
    assert old["stats"].shape == (7, 5, 512) and new["stats"].shape == (7, 5, 512)
    assert "fa_stats" not in old and "spec_stats" not in old
    for k in ("stats", "sigma", "rep_status", "fsol", "sig", "reg", "lam", "maps", "status"):
        assert torch.equal(old[k], new[k]), k
    assert bool(((new["status"] & 1) != 0).all())
    fs = new["fa_stats"]
    assert fs.shape == (5, 512) and new["spec_stats"].shape == (5, 512, 60)
    for i in (0, 2, 3, 4):
        assert torch.equal(fs[i], fa_true), i
    assert bool((fs[1] == 0.0).all())
    deg = new["fa_stats_deg"]
    assert np.array_equal(deg[0], P.alphas[fa_true.cpu().numpy().astype(int)]) and np.all(deg[1] == 0.0)
    P.close()


CASES = [("X2", "L2", 32, 60, "brute-force", 512, 32), ("GCV", "L2", 48, 120, "brute-force", 512, 32), ("L_curve", "L1", 32, 60, "spline", 512, 32),
         ("BayesReg", "InvT2", 32, 60, "brute-force", 512, 32), ("X2", "L2", 32, 60, "brute-force", 512, 33),
         ("X2", "L2", 48, 120, "brute-force", 8, 1024)]


@pytest.mark.parametrize("method,penalty,nte,nt2,fa,nvox,B", CASES)
def test_fused_equals_composed(pkg, synth, method, penalty, nte, nt2, fa, nvox, B):
    P = Plans(pkg, synth, nte, nt2, penalty, fa)
    plan = P.plan
    data, _, _ = synth.make_voxels(nvox, nte=nte, seed=32, fa_values=P.alphas, device="cuda:0")
    seed = 78
    fa_point = P.estimate(data)
    out = plan.fit_bootstrap(method, data, n_rep=B, seed=seed, fa_index=fa_point, want_lambda=True, fa=fa, want_spectrum=True)
    ref = plan.fit(method, data, fa_index=fa_point, want_lambda=True)
    for k in ("fsol", "sig", "reg", "lam", "maps", "status"):
        assert torch.equal(out[k], ref[k]), k
    fitted = (out["status"] & 1) != 0
    assert bool(fitted.all())
    rows = plan.bootstrap_replicates(out["sig"], out["sigma"], B, seed).reshape(nvox * B, nte)
    mrows = fitted.repeat_interleave(B)
    fa_rows = P.estimate(rows, mrows)
    fr = plan.fit(method, rows, fa_index=fa_rows, mask=mrows)
    vals = torch.cat([fr["maps"], fr["reg"][None], fa_rows[None]], 0).reshape(8, nvox, B).cpu().numpy()
    got = torch.cat([out["stats"], out["fa_stats"][None]], 0).cpu().numpy()                    # [8, 5, nvox]
    check_stats(np.moveaxis(got, 0, 1), vals, "stats")
    spectra = fr["fsol"].reshape(nvox, B, nt2).permute(0, 2, 1).cpu().numpy()                   # [nvox, nt2, B]
    check_stats(out["spec_stats"].cpu().numpy(), spectra, "spec_stats")
    st = fr["status"].reshape(nvox, B).cpu().numpy()
    assert np.array_equal(out["rep_status"].cpu().numpy(), np.bitwise_or.reduce(st, axis=1))
    assert len(np.unique(vals[7])) > 1                                                            # the walk found different angles
    P.close()


def test_invariance_to_splitting_and_order(pkg, synth):
    P = Plans(pkg, synth)
    plan = P.plan
    data, _, _ = synth.make_voxels(3000, nte=32, seed=33, fa_values=P.alphas, device="cuda:0")
    fa_point = P.estimate(data)
    B, seed = 24, 2 ** 40 + 3
    kw = dict(n_rep=B, seed=seed, fa="brute-force", want_spectrum=True)
    keys = ("stats", "fa_stats", "rep_status", "sigma")
    one = plan.fit_bootstrap("X2", data, fa_index=fa_point, **kw)
    two = plan.fit_bootstrap("X2", data, fa_index=fa_point, **kw)
    for k in keys + ("spec_stats",):
        assert torch.equal(one[k], two[k]), k
    cuts = [0, 1000, 1001, 3000]
    parts = [plan.fit_bootstrap("X2", data[a:b].contiguous(), fa_index=fa_point[a:b], voxel_id=np.arange(a, b), **kw)
             for a, b in zip(cuts[:-1], cuts[1:])]
    for k in keys:
        assert torch.equal(one[k], torch.cat([p[k] for p in parts], dim=-1)), k
    assert torch.equal(one["spec_stats"], torch.cat([p["spec_stats"] for p in parts], dim=1))
    perm = torch.as_tensor(np.random.default_rng(3).permutation(3000), device="cuda:0")
    pm = plan.fit_bootstrap("X2", data[perm].contiguous(), fa_index=fa_point[perm], voxel_id=perm, **kw)
    for k in keys:
        assert torch.equal(one[k][..., perm], pm[k]), k
    assert torch.equal(one["spec_stats"][:, perm], pm["spec_stats"])
    P.close()


def test_gated_voxels_get_zero_stats(pkg, synth):
    P = Plans(pkg, synth)
    data, _, _ = synth.make_voxels(256, nte=32, seed=34, fa_values=P.alphas, device="cuda:0")
    data[1] = 0.0
    data[2, 5] = float("nan")
    mask = torch.ones(256, dtype=torch.uint8, device="cuda:0")
    mask[0] = 0
    fa_point = P.estimate(torch.nan_to_num(data), mask)
    out = P.plan.fit_bootstrap("X2", data, n_rep=8, seed=4, mask=mask, fa_index=fa_point, fa="brute-force", want_spectrum=True)
    ref = P.plan.fit("X2", data, mask=mask, fa_index=fa_point)
    assert torch.equal(out["status"], ref["status"])
    for k in ("fsol", "reg", "maps"):
        assert torch.equal(out[k], ref[k]), k
    st = torch.cat([out["stats"], out["fa_stats"][None]], 0).cpu().numpy()
    sp = out["spec_stats"].cpu().numpy()
    assert np.all(st[:, :, :3] == 0.0) and np.all(sp[:, :3] == 0.0) and np.all(out["rep_status"][:3].cpu().numpy() == 0)
    assert np.all(st[5, 1, 3:] > 0.0) and np.all((out["rep_status"][3:].cpu().numpy() & 1) == 1)
    assert np.all(sp[0, 3:].sum(-1) > 0.0)
    P.close()


def chunk_voxels(method, nt2, n_rep, nvox):
    """voxels per internal chunk as include/met2_hip.h states them: whole voxels within 262 144 replicate rows, 4 096 for L-curve at n_t2 > 64"""
    rmax = 4096 if method == "L_curve" and nt2 > 64 else 262144
    return min(nvox, max(1, rmax // n_rep))


BOOT_KEYS = ("stats", "fa_stats", "rep_status", "sigma")
# method, penalty, nte, nt2, fa, nvox, B, the chunks the call is expected to make, where the split calls cut
CHUNK_CASES = [("X2", "L2", 32, 60, "brute-force", 300, 1024, [256, 44], [0, 100, 256, 257, 300]),
               ("X2", "L2", 32, 60, "spline", 300, 1000, [262, 38], [0, 261, 262, 300]),         # aux is sized by the first chunk, reused by a smaller one
               ("L_curve", "L1", 48, 120, "brute-force", 400, 24, [170, 170, 60], [0, 90, 170, 341, 400])]


@pytest.mark.parametrize("method,penalty,nte,nt2,fa,nvox,B,chunks,cuts", CHUNK_CASES)
def test_chunk_edges_fused_equals_composed_and_split(pkg, synth, method, penalty, nte, nt2, fa, nvox, B, chunks, cuts):
    """A call of several chunks with a partial last one: the chunk-local row index against the global voxel index in both statistics kernels,
    the FA row, the spectrum and the spline mode's residual buffer.  Fused against composed with check_stats, and against the same voxels
    fitted in calls cut inside chunks and at their boundaries, bit for bit."""
    vpc = chunk_voxels(method, nt2, B, nvox)
    assert [min(vpc, nvox - v0) for v0 in range(0, nvox, vpc)] == chunks and len(chunks) > 1 and chunks[-1] < vpc       # the premise
    assert any(c % vpc == 0 for c in cuts[1:-1]) and any(c % vpc != 0 for c in cuts[1:-1])
    P = Plans(pkg, synth, nte, nt2, penalty, fa)
    plan = P.plan
    data, _, _ = synth.make_voxels(nvox, nte=nte, seed=41, fa_values=P.alphas, device="cuda:0")
    seed = 2 ** 33 + 5
    fa_point = P.estimate(data)
    kw = dict(n_rep=B, seed=seed, fa=fa, want_spectrum=True)
    one = plan.fit_bootstrap(method, data, fa_index=fa_point, **kw)
    assert bool(((one["status"] & 1) != 0).all())
    # composed: the fits in runs of 4 096 rows, which are not the call's chunks (and which L-curve at two bins per lane needs: past them the
    # spill-over kernel's outcome may depend on arrival order)
    rows = plan.bootstrap_replicates(one["sig"], one["sigma"], B, seed).reshape(nvox * B, nte)
    fa_rows = P.estimate(rows)
    step = 4096 if method == "L_curve" else nvox * B
    frs = [plan.fit(method, rows[a:a + step].contiguous(), fa_index=fa_rows[a:a + step]) for a in range(0, nvox * B, step)]
    fr = {k: torch.cat([f[k] for f in frs], dim=-1 if k != "fsol" else 0) for k in ("maps", "reg", "fsol", "status")}
    vals = torch.cat([fr["maps"], fr["reg"][None], fa_rows[None]], 0).reshape(8, nvox, B).cpu().numpy()
    got = torch.cat([one["stats"], one["fa_stats"][None]], 0).cpu().numpy()                      # [8, 5, nvox]
    check_stats(np.moveaxis(got, 0, 1), vals, "stats over %d chunks" % len(chunks))
    spectra = fr["fsol"].reshape(nvox, B, nt2).permute(0, 2, 1).cpu().numpy()                     # [nvox, nt2, B]
    check_stats(one["spec_stats"].cpu().numpy(), spectra, "spec_stats over %d chunks" % len(chunks))
    st = fr["status"].reshape(nvox, B).cpu().numpy()
    assert np.array_equal(one["rep_status"].cpu().numpy(), np.bitwise_or.reduce(st, axis=1))
    assert len(np.unique(vals[7, vpc:])) > 1                                                      # the walk found different angles past the first chunk
    del rows, frs, fr
    # the same voxels in several calls
    parts = [plan.fit_bootstrap(method, data[a:b].contiguous(), fa_index=fa_point[a:b], voxel_id=np.arange(a, b), **kw)
             for a, b in zip(cuts[:-1], cuts[1:])]
    for k in BOOT_KEYS:
        assert torch.equal(one[k], torch.cat([p[k] for p in parts], dim=-1)), k
    assert torch.equal(one["spec_stats"], torch.cat([p["spec_stats"] for p in parts], dim=1))
    P.close()


def test_gated_voxels_in_the_second_chunk(pkg, synth):
    """A masked voxel, an all-zero voxel and a voxel with a nan echo past the first chunk: zeros for them (pstatus[v] is read at the global
    index), and the rest of that chunk as a call of its own gives it."""
    nvox, B, nt2 = 300, 1024, 60
    vpc = chunk_voxels("X2", nt2, B, nvox)
    gated = [vpc + 4, vpc + 14, nvox - 1]
    assert vpc < min(gated) and nvox % vpc != 0                                                   # the premise: all three in a partial second chunk
    P = Plans(pkg, synth)
    data, _, _ = synth.make_voxels(nvox, nte=32, seed=42, fa_values=P.alphas, device="cuda:0")
    mask = torch.ones(nvox, dtype=torch.uint8, device="cuda:0")
    mask[gated[0]] = 0
    data[gated[1]] = 0.0
    data[gated[2], 5] = float("nan")
    fa_point = P.estimate(torch.nan_to_num(data), mask)
    kw = dict(n_rep=B, seed=4, fa="brute-force", want_spectrum=True)
    out = P.plan.fit_bootstrap("X2", data, mask=mask, fa_index=fa_point, **kw)
    ref = P.plan.fit("X2", data, mask=mask, fa_index=fa_point)
    assert torch.equal(out["status"], ref["status"])
    fitted = ((out["status"] & 1) != 0).cpu().numpy()
    assert np.array_equal(np.where(~fitted)[0], gated)
    st = torch.cat([out["stats"], out["fa_stats"][None]], 0).cpu().numpy()
    sp = out["spec_stats"].cpu().numpy()
    rs = out["rep_status"].cpu().numpy()
    assert np.all(st[:, :, gated] == 0.0) and np.all(sp[:, gated] == 0.0) and np.all(rs[gated] == 0)
    assert np.all(st[5, 1, fitted] > 0.0) and np.all((rs[fitted] & 1) == 1) and np.all(sp[0, fitted].sum(-1) > 0.0)
    tail = P.plan.fit_bootstrap("X2", data[vpc:].contiguous(), mask=mask[vpc:], fa_index=fa_point[vpc:], voxel_id=np.arange(vpc, nvox), **kw)
    for k in ("stats", "fa_stats", "rep_status"):
        assert torch.equal(out[k][..., vpc:], tail[k]), k
    ft = torch.as_tensor(fitted[vpc:], device="cuda:0")                                          # sigma of the voxel with a nan echo is nan
    assert torch.equal(out["sigma"][vpc:][ft], tail["sigma"][ft])
    assert torch.equal(out["spec_stats"][:, vpc:], tail["spec_stats"])
    P.close()


def test_spline_mode_needs_an_attached_coarse_plan(pkg, synth):
    lib = importlib.import_module(PKG + "._lib")
    P = Plans(pkg, synth, fa="spline", attach=False)
    data, fa_true, _ = synth.make_voxels(64, nte=32, seed=35, fa_values=P.alphas, device="cuda:0")
    with pytest.raises(lib.Met2Error, match="attach_fa_spline"):
        P.plan.fit_bootstrap("X2", data, n_rep=8, seed=1, fa_index=fa_true, fa="spline")
    P.plan.attach_fa_spline(P.coarse, P.alpha_lr)
    out = P.plan.fit_bootstrap("X2", data, n_rep=8, seed=1, fa_index=fa_true, fa="spline")
    assert out["fa_stats"].shape == (5, 64) and "spec_stats" not in out
    P.plan.attach_fa_spline(None, None)
    with pytest.raises(lib.Met2Error, match="attach_fa_spline"):
        P.plan.fit_bootstrap("X2", data, n_rep=8, seed=1, fa_index=fa_true, fa="spline")
    with pytest.raises(ValueError, match="fa must be"):
        P.plan.fit_bootstrap("X2", data, n_rep=8, seed=1, fa_index=fa_true, fa="smoothed")
    P.close()


def test_sigma_zero_gives_degenerate_bands(pkg, synth):
    P = Plans(pkg, synth)
    data, _, _ = synth.make_voxels(512, nte=32, seed=36, fa_values=P.alphas, device="cuda:0")
    fa_point = P.estimate(data)
    z = P.plan.fit_bootstrap("X2", data, n_rep=16, seed=21, sigma=torch.zeros(512, dtype=torch.float64, device="cuda:0"), fa_index=fa_point,
                             fa="brute-force", want_spectrum=True)
    sp = z["spec_stats"].cpu().numpy()
    assert np.all(sp[1] == 0.0)
    assert np.array_equal(sp[0], sp[3]) and np.array_equal(sp[2], sp[3]) and np.array_equal(sp[3], sp[4])
    assert np.any(sp[0] > 0.0)
    fs = z["fa_stats"].cpu().numpy()
    assert np.all(fs[1] == 0.0) and np.array_equal(fs[0], fs[3]) and np.array_equal(fs[2], fs[4])
    st = z["stats"].cpu().numpy()
    assert np.all(st[:, 1] == 0.0)
    P.close()


def test_volume_layouts(pkg, synth):
    P = Plans(pkg, synth)
    data, _, _ = synth.make_voxels(6 * 5 * 4, nte=32, seed=37, fa_values=P.alphas, device="cuda:0")
    vol = data.reshape(6, 5, 4, 32)
    fvol = vol.permute(3, 2, 1, 0).contiguous().permute(3, 2, 1, 0)            # Fortran order, as nibabel's arrays
    vid = np.arange(120).reshape(6, 5, 4)
    fa_point = P.estimate(data).reshape(6, 5, 4)
    kw = dict(n_rep=8, seed=6, voxel_id=vid, fa_index=fa_point, fa="brute-force", want_spectrum=True)
    c = P.plan.fit_bootstrap("X2", vol, **kw)
    f = P.plan.fit_bootstrap("X2", fvol, **kw)
    assert c["stats"].shape == (7, 5, 6, 5, 4) and c["fa_stats"].shape == (5, 6, 5, 4) and c["spec_stats"].shape == (5, 6, 5, 4, 60)
    assert c["fa_stats_deg"].shape == (5, 6, 5, 4)
    for k in ("stats", "fa_stats", "spec_stats", "sigma", "rep_status", "maps"):
        assert torch.equal(c[k], f[k]), k
    assert np.array_equal(c["fa_stats_deg"], f["fa_stats_deg"])
    P.close()


NEW_FILES = ["FA_bootstrap.nii.gz"] + ["fsol_bootstrap_%s.nii.gz" % s for s in ("mean", "std", "q025", "q500", "q975")]


def test_drivers(pkg, synth, tmp_path):
    motor = importlib.import_module(PKG + ".motor")
    nifti = importlib.import_module(PKG + ".nifti")
    data, mask = synth.make_phantom((10, 9, 6), nte=32, seed=38)
    d, m = data.cpu().numpy(), mask.cpu().numpy()
    TE = 10.0 * np.arange(1, 33)
    names = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param")
    bs = dict(n_rep=8, seed=1, fa="brute-force", spectrum=True)
    plain = motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", "brute-force", 40.0, FA_smooth="no")
    boot = motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", bootstrap=bs, FA_method="brute-force", FA_smooth="no")
    for k in names:
        assert np.array_equal(plain[k], boot[k]), k
    assert boot["FA_bootstrap"].shape == (10, 9, 6, 5) and boot["fsol_bootstrap"].shape == (10, 9, 6, 60, 5)
    # a direct call on the prepared volume with the run's flip angles
    P = Plans(pkg, synth)
    dd = torch.as_tensor(np.where(d * m[..., None] < 0, 0.0, d * m[..., None]), device="cuda:0")
    out = P.plan.fit_bootstrap("X2", dd, n_rep=8, seed=1, fa_index=boot["FA_index"], mask=m > 0, voxel_id=np.arange(540).reshape(10, 9, 6),
                               fa="brute-force", want_spectrum=True)
    fitted = (out["rep_status"].cpu().numpy() != 0)[..., None]
    assert np.array_equal(boot["FA_bootstrap"], np.where(fitted, np.moveaxis(out["fa_stats_deg"], 0, -1), 0.0))
    assert np.array_equal(boot["fsol_bootstrap"], np.moveaxis(out["spec_stats"].cpu().numpy(), 0, -1))
    stats = out["stats"].cpu().numpy()
    for i, q in enumerate(pkg.BOOT_QUANTITIES):
        assert np.array_equal(boot[q + "_bootstrap"], np.moveaxis(stats[i], 0, -1)), q
    inside = m > 0
    assert np.all(boot["FA_bootstrap"][~inside] == 0.0) and np.all(boot["fsol_bootstrap"][~inside] == 0.0)
    assert np.all(boot["FA_bootstrap"][inside][:, 0] >= 90.0)
    P.close()
    with pytest.raises(ValueError, match="FA_smooth"):
        motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", bootstrap=bs, FA_method="brute-force", FA_smooth="yes")
    # without the new keys nothing new is returned
    old = motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", "brute-force", 40.0, bootstrap=dict(n_rep=8, seed=1))
    assert "FA_bootstrap" not in old and "fsol_bootstrap" not in old
    # the spline pipeline builds and attaches its own coarse plan
    spl = motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", "spline", 40.0, FA_smooth="no", bootstrap=dict(n_rep=8, seed=1, fa="spline"))
    assert spl["FA_bootstrap"].shape == (10, 9, 6, 5) and "fsol_bootstrap" not in spl
    assert np.all(spl["FA_bootstrap"][inside][:, 0] >= 90.0)
    # files
    aff = np.diag([1.5, 1.5, 3.0, 1.0])
    nifti.save(nifti.NiftiImage(np.asfortranarray(d), aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(m.astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    a = str(tmp_path) + "/a_"
    res = motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), a, 3000.0, "X2", "L2", "None",
                                 "brute-force", "no", 40.0, bootstrap=bs)
    got = nifti.load(a + "FA_bootstrap.nii.gz").get_fdata()
    assert got.shape == (10, 9, 6, 5) and np.array_equal(got, res["FA_bootstrap"]) and np.array_equal(got, boot["FA_bootstrap"])
    for i, s in enumerate(pkg.BOOT_STATS):
        got = nifti.load(a + "fsol_bootstrap_%s.nii.gz" % s).get_fdata()
        assert got.shape == (10, 9, 6, 60) and np.array_equal(got, boot["fsol_bootstrap"][..., i]), s
    b = str(tmp_path) + "/b_"
    motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), b, 3000.0, "X2", "L2", "None",
                           "brute-force", "no", 40.0, bootstrap=dict(n_rep=8, seed=1))
    assert os.path.exists(b + "MWF_bootstrap.nii.gz")
    for f in NEW_FILES:
        assert os.path.exists(a + f) and not os.path.exists(b + f), f


def test_what_the_spread_means(pkg, synth):
    """Not a tolerance test.  Empirical std of the MWF over R independent Rician draws, each with its flip angle re-estimated by the
    brute-force walk, against the bootstrap std of ONE draw in both modes; the two medians of bootstrap / empirical are printed (to be
    recorded in profiles/boot_fa_spread.txt; on an MI355X: 0.955 with the FA fixed, 1.012 with it re-estimated).  Asserted: only that the re-estimating mode did re-estimate."""
    P = Plans(pkg, synth)
    plan = P.plan
    n, snr, R = 2048, 100.0, 64
    clean, _, _ = synth.make_voxels(n, nte=32, seed=16, snr=(1e15, 1e15), fa_values=P.alphas, device="cuda:0")     # noise-free to ~1e-15
    sg = clean[:, :1] / snr
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(5)
    draws = [torch.sqrt((clean + sg * torch.randn(clean.shape, dtype=torch.float64, device="cuda:0", generator=gen)) ** 2 +
                        (sg * torch.randn(clean.shape, dtype=torch.float64, device="cuda:0", generator=gen)) ** 2) for _ in range(R)]
    fas = [plan.fa_bruteforce(d)[0] for d in draws]
    mwf = torch.stack([plan.fit("X2", d, fa_index=f, want_sig=False)["maps"][0] for d, f in zip(draws, fas)]).cpu().numpy()     # [R, n]
    emp = mwf.std(0, ddof=1)
    emp_fa = torch.stack(fas).cpu().numpy().std(0, ddof=1)
    ok = emp > 0
    res = {}
    for mode in ("fixed", "brute-force"):
        out = plan.fit_bootstrap("X2", draws[0], n_rep=64, seed=21, sigma=sg[:, 0], fa_index=fas[0], fa=mode, want_spectrum=False)
        boot = out["stats"][0, 1].cpu().numpy()
        res[mode] = out
        print("fa=%-11s median bootstrap / empirical std(MWF) = %.3f" % (mode, np.median(boot[ok] / emp[ok])))
    fa_sd = res["brute-force"]["fa_stats"][1].cpu().numpy()
    print("median empirical std(FA index) = %.3f, median bootstrap std(FA index) = %.3f" % (np.median(emp_fa), np.median(fa_sd)))
    assert "fa_stats" not in res["fixed"]          # fixed mode without the spectrum is the older entry: no replicate got another angle
    assert np.any(fa_sd > 0.0)                     # some voxel's replicates were fitted at more than one flip angle
    P.close()
