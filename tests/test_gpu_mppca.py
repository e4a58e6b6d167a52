"""GPU tests of met2_mppca (csrc/met2_mppca.hip) and of denoise='MPPCA' in the drivers, against the numpy restatement of the algorithm
(tests/tools/mppca_numpy.py: np.linalg.eigh and the threshold loop of include/met2_hip.h).

Tolerances.  The rank is a discrete decision, so a voxel may be left out of a comparison only where the restatement itself calls the decision a
tie (margin < 1e-6 or gap < 1e-6, mppca_numpy.ties), at most 1 % of the voxels, asserted -- and tests/test_mppca_host.py asserts that on
the volumes used here the restatement calls none.  On all others: rank equal; |out - ref| <= 1e-9 max|data|; |sigma - ref| <= 1e-6 ref.
These come from perturbing C by a random symmetric matrix of 1e-14 ||C||_2 (10-50 times a Jacobi's backward error) on such volumes: out moved
by 4e-11 max|data|, sigma by 1.2e-8 relative, no rank changed.

Shapes are the smallest at which the kernel takes another path: patches with fewer (N = 27 at corners) and more (125) voxels than echoes,
odd echo counts (a dummy player in the tournament), echo counts at which two or more pairs are rotated side by side (<= 32) or one (>= 33),
the maximum 63, windows clipped on every side."""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mppca_numpy as mp                                           # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def motor():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".motor")


@pytest.fixture(scope="module")
def stages(motor):
    return importlib.import_module(PKG + ".mppca").mppca_stages


@functools.lru_cache(maxsize=None)
def reference(name):
    """(data, mask, window, restatement's result) of a committed case: computed once, shared, never written to"""
    data, mask, w = mp.case(name)
    res = mp.mppca(data, mask, w)
    for a in (data, mask) + tuple(res.values()):
        a.setflags(write=False)
    return data, mask, w, res


def check_against(ref, data, out, sigma, rank, where=None):
    tie = mp.ties(ref)
    use = ~tie if where is None else (~tie & where)
    n = int(np.prod(tie.shape))
    print("ties left out: %d of %d" % (int(tie.sum()), n))
    assert tie.sum() <= 0.01 * n
    scale = np.abs(data[np.isfinite(data)]).max()
    e_out = np.abs(out[use] - ref["out"][use]).max() / scale
    rs = ref["sigma"][use]
    e_sig = np.max(np.abs(sigma[use] - rs) / np.where(rs > 0, rs, 1.0))
    print("max |out - ref| / max|data| = %.3e, max rel |sigma - ref| = %.3e, ranks %s" % (e_out, e_sig, np.unique(rank[use])))
    assert np.array_equal(rank[use], ref["rank"][use])
    assert e_out <= 1e-9
    assert np.all(np.abs(sigma[use] - rs) <= 1e-6 * rs)


def test_parity_with_the_restatement(motor):
    data, mask, w, ref = reference("parity")
    assert ref["n"].max() == 125 and ref["n"][mask != 0].min() <= 27 < 32          # both branches of r and q
    out, sigma, rank = motor.mppca_filter(data, mask, window=w, return_maps=True)
    assert not out[mask == 0].any() and not sigma[mask == 0].any() and not rank[mask == 0].any()
    check_against(ref, data, out, sigma, rank)
    # CUDA tensors in, tensors out; without the maps the same volume
    t = motor.mppca_filter(torch.as_tensor(data, device="cuda"), torch.as_tensor(mask, device="cuda"), window=w)
    assert torch.is_tensor(t) and t.is_cuda and np.array_equal(t.cpu().numpy(), out)


@pytest.mark.parametrize("name", ["M2", "M7", "M16", "M33", "M63", "M3", "M21", "M22", "M31", "M62"])
def test_echo_count_edges(motor, name):
    # G = floor(64 / M) pairs are rotated side by side: it changes at M = 3 (two pairs in G = 21), 21 -> 22 (G = 3 -> 2), 32 -> 33 (2 -> 1);
    # 31 and 63 are odd (a dummy player), 62 is the even maximum
    data, mask, w, ref = reference(name)
    out, sigma, rank = motor.mppca_filter(data, mask, window=w, return_maps=True)
    check_against(ref, data, out, sigma, rank)


def test_window_7_at_63_echoes(motor):
    # the longest patch list that fits (4 * 343 bytes, past the 1024 bytes the rotations and the spectrum share with it) on data that is not zero
    data, mask, w, ref = reference("W7M63")
    assert w == 7 and data.shape[-1] == 63 and ref["n"].max() > 256
    out, sigma, rank = motor.mppca_filter(data, mask, window=w, return_maps=True)
    check_against(ref, data, out, sigma, rank)


@pytest.mark.parametrize("name", ["parity", "M33"])
@pytest.mark.parametrize("e", [40, -40])
def test_scaling_by_a_power_of_two_is_exact(stages, name, e):
    # every operation of the kernel commutes with a power of two short of over- and underflow (the sigma's square root too: the exponent is even)
    data, mask, w, ref = reference(name)
    a = stages(data, mask, window=w)
    b = stages(np.ldexp(data, e), mask, window=w)
    assert np.array_equal(b["out"], np.ldexp(a["out"], e)) and np.array_equal(b["sigma"], np.ldexp(a["sigma"], e))
    assert np.array_equal(b["rank"], a["rank"]) and np.array_equal(b["sweeps"], a["sweeps"])
    assert (a["rank"][mask != 0] > 0).any()


def test_products_of_diagonal_entries_that_overflow(motor, stages):
    # parity x 2^250: C is finite (about 2^550), c_pp c_qq is not; the rotation test must not take +inf for its threshold
    data, mask, w, ref = reference("parity")
    base = motor.mppca_filter(data, mask, window=w, return_maps=True)
    big = stages(np.ldexp(data, 250), mask, window=w)
    assert np.isfinite(big["gram"]).all() and np.ldexp(big["gram"], -500).max() > 1e6
    assert np.array_equal(big["rank"], base[2])
    scale = np.abs(data).max()
    e_out = np.abs(np.ldexp(big["out"], -250) - base[0]).max() / scale
    print("max |out / 2^250 - out| / max|data| = %.3e" % e_out)
    assert e_out <= 1e-9
    worst = {}
    M = data.shape[-1]
    gram, ev, V = (big[k].reshape((-1,) + big[k].shape[3:]) for k in ("gram", "eigval", "eigvec"))
    ran = np.flatnonzero((big["n_patch"].reshape(-1) >= 2) & (big["rank"].reshape(-1) >= 0))
    assert ran.size == int((big["n_patch"] >= 2).sum())
    for v in ran:
        Cm = np.ldexp(gram[v], -500)                               # exact: the figures are relative
        bounds, _ = mp.eig_bounds(Cm)
        got = mp.eig_figures(Cm, np.ldexp(ev[v], -500), V[v])
        for k in got:
            worst[k] = max(worst.get(k, 0.0), got[k] / bounds[k])
            assert got[k] <= bounds[k], (v, k, got[k], bounds[k])
    print("max figure / bound:", {k: "%.3f" % x for k, x in worst.items()})
    assert (big["sweeps"][big["rank"] > 0] > 1).all()


def test_gram_matrix_that_overflows(stages):
    # parity x 2^520: the data are finite, C is not: every voxel is copied through with rank -1
    data, mask, w, ref = reference("parity")
    huge = np.ldexp(data, 520)
    assert np.isfinite(huge).all()
    res = stages(huge, mask, window=w)
    on = (mask != 0) & (ref["n"] >= 2)
    assert (res["rank"][on] == -1).all() and not res["sigma"].any()
    assert np.array_equal(res["out"], huge)
    out, sigma, rank = importlib.import_module(PKG + ".motor").mppca_filter(huge, mask, window=w, return_maps=True)
    assert np.array_equal(out, huge) and np.array_equal(rank, res["rank"]) and not sigma.any()


@pytest.mark.parametrize("name", ["wide", "tiny"])
def test_window_wider_than_the_volume(motor, name):
    data, mask, w, ref = reference(name)
    assert any(w > n for n in data.shape[:3]) or data.shape[:3] == (2, 2, 2)
    out, sigma, rank = motor.mppca_filter(data, mask, window=w, return_maps=True)
    check_against(ref, data, out, sigma, rank)


def test_special_cases(motor):
    data, mask, w, ref = reference("parity")
    # an isolated mask voxel: N = 1, copied through, rank 1
    m1 = np.zeros_like(mask)
    m1[4, 4, 3] = 1
    m1[0, 0, 0] = 1
    out, sigma, rank = motor.mppca_filter(data, m1, window=3, return_maps=True)
    for v in ((4, 4, 3), (0, 0, 0)):
        assert np.array_equal(out[v], data[v]) and sigma[v] == 0.0 and rank[v] == 1
    assert rank.sum() == 2 and not out[m1 == 0].any()
    # an all-zero patch: zeros, sigma 0, no failure code
    full = np.ones_like(mask)
    zero = np.array(data)
    zero[:5, :5, :5] = 0.0
    out, sigma, rank = motor.mppca_filter(zero, full, window=3, return_maps=True)
    assert not out[:4, :4, :4].any() and not sigma[:4, :4, :4].any() and (rank[:4, :4, :4] >= 0).all()
    # one NaN and one Inf: exactly the voxels whose patch holds one are copied through with rank -1, every other voxel is what a run with
    # the two voxels masked out gives (its patch never held them)
    bad = np.array(data)
    bad[2, 2, 2, 5] = np.nan
    bad[7, 6, 5, 31] = np.inf
    out, sigma, rank = motor.mppca_filter(bad, full, window=w, return_maps=True)
    hit = np.zeros(mask.shape, dtype=bool)
    hit[0:5, 0:5, 0:5] = True
    hit[5:9, 4:8, 3:7] = True
    assert np.array_equal(rank == -1, hit)
    assert np.array_equal(out[hit], bad[hit], equal_nan=True) and not sigma[hit].any()
    m2 = np.array(full)
    m2[2, 2, 2] = 0
    m2[7, 6, 5] = 0
    out2, sigma2, rank2 = motor.mppca_filter(bad, m2, window=w, return_maps=True)
    assert (rank2 >= 0).all()
    assert np.array_equal(out[~hit], out2[~hit]) and np.array_equal(sigma[~hit], sigma2[~hit]) and np.array_equal(rank[~hit], rank2[~hit])
    # sigma and rank NULL: the same volume
    lib = importlib.import_module(PKG + "._lib")
    dd = torch.as_tensor(data, device="cuda").contiguous()
    mk = torch.as_tensor(mask, device="cuda").contiguous()
    o = torch.empty_like(dd)
    nx, ny, nz, nt = dd.shape
    assert lib.lib().met2_mppca(0, nx, ny, nz, nt, dd.data_ptr(), mk.data_ptr(), w, o.data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), motor.mppca_filter(data, mask, window=w))


def test_deterministic_and_independent_of_the_rest_of_the_volume(motor):
    data, mask, w, ref = reference("parity")
    a = motor.mppca_filter(data, mask, window=w, return_maps=True)
    b = motor.mppca_filter(data, mask, window=w, return_maps=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # a voxel's output does not change when the volume is cropped to exactly its patch (the patch list keeps its memory order)
    for (x, y, z) in ((4, 4, 3), (0, 1, 1), (8, 7, 6), (6, 2, 0)):
        sl = tuple(slice(max(c - w // 2, 0), min(c + w // 2 + 1, n)) for c, n in zip((x, y, z), mask.shape))
        at = tuple(c - s.start for c, s in zip((x, y, z), sl))
        assert mask[x, y, z]
        c = motor.mppca_filter(np.ascontiguousarray(data[sl]), np.ascontiguousarray(mask[sl]), window=w, return_maps=True)
        for full, crop in zip(a, c):
            assert np.array_equal(full[x, y, z], crop[at]), (x, y, z)


def test_driver_takes_denoise_mppca(motor, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    data, mask, w, ref = reference("driver")
    assert w == 5                                                   # the driver's window
    TE = 10.0 * np.arange(1, data.shape[-1] + 1)
    raw = np.array(data)
    raw[1, 2, 3, 30] = -5.0                                         # clipped before the filter (motor:279)
    got = motor.recon_met2_arrays(raw, mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0, denoise="MPPCA", return_prepared=True)
    prep = raw * mask[..., None]
    prep = np.where(prep < 0, 0.0, prep)
    den, sigma, rank = motor.mppca_filter(prep, mask, window=5, return_maps=True)
    den = np.where(den < 0, 0.0, den)
    assert np.array_equal(got["data_prepared"], den) and np.array_equal(got["MPPCA_sigma"], sigma)
    want = motor.recon_met2_arrays(den, mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0, prepared=True)
    keys = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param")
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert want["MWF"][mask != 0].max() > 0.0
    # the devices=[...] leg, spelt out, and without return_prepared: the ten outputs and nothing of the filter's
    multi = motor.recon_met2_arrays(raw, mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0, denoise="MPPCA", devices=[0])
    assert "MPPCA_sigma" not in multi and "data_prepared" not in multi
    for k in keys:
        assert np.array_equal(multi[k], want[k], equal_nan=True), k
    # the on-disk driver: the ten volumes, the denoised data and the noise map
    aff = np.eye(4)
    nifti.save(nifti.NiftiImage(raw, aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(mask.astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/mp_"
    motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "MPPCA", "brute-force", "no",
                           40.0, 1)
    assert np.array_equal(nifti.load(out + "MPPCA_sigma.nii.gz").get_fdata(), sigma)
    assert np.array_equal(nifti.load(out + "Data_denoised.nii.gz").get_fdata(), den)
    assert np.array_equal(nifti.load(out + "MWF.nii.gz").get_fdata(), want["MWF"])
    for k in keys:
        assert os.path.exists(out + k + ".nii.gz"), k
    with pytest.raises(ValueError, match="MPPCA"):
        motor.recon_met2_arrays(raw, mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0, denoise="PCA")


def test_return_codes(motor):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    dd = torch.zeros((3, 3, 3, 64), dtype=torch.float64, device="cuda")
    mk = torch.ones((3, 3, 3), dtype=torch.uint8, device="cuda")
    o = torch.empty_like(dd)
    call = lambda nt, w, out=o, shape=(3, 3, 3): L.met2_mppca(0, shape[0], shape[1], shape[2], nt, dd.data_ptr(), mk.data_ptr(), w,
                                                              None if out is None else out.data_ptr(), None, None, None)
    assert call(32, 4) == E_INVALID
    assert call(32, 1) == E_INVALID
    assert call(32, 5, out=None) == E_INVALID
    assert call(64, 5) == E_UNSUPPORTED
    assert call(1, 5) == E_UNSUPPORTED
    assert call(63, 9) == E_UNSUPPORTED                             # 4 * 9^3 bytes of patch list beside two 63 x 63 matrices: more than 64 KB
    o.fill_(7.0)
    assert call(32, 5, shape=(0, 3, 3)) == 0
    assert L.met2_mppca(0, 0, 3, 3, 32, None, None, 5, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                   # nothing was launched
    assert call(63, 7) == 0                                         # the largest region that fits
    torch.cuda.synchronize()
    with pytest.raises(lib.Met2Error):
        motor.mppca_filter(np.zeros((3, 3, 3, 8)), np.ones((3, 3, 3)), window=2)
    with pytest.raises(ValueError):
        motor.mppca_filter(np.zeros((3, 3, 8)), np.ones((3, 3, 3)))
