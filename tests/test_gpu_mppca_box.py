"""GPU tests of met2_mppca_box (csrc/met2_mppca.hip: MP-PCA with a box window and the average over the overlapping patches) and of
mppca_filter(window=, average=) and the drivers' denoise={...} in front of it, against met2_mppca where the two must agree to the bit and against the numpy restatement
(tests/tools/mppca_box_numpy.py) everywhere else.

Tolerances: those tests/test_gpu_mppca.py holds met2_mppca to (MP-PCA row) -- n_patch and rank equal, |out - ref| <= 1e-9
max|data|, |sigma - ref| <= 1e-6 ref -- and |wsum - ref| <= 1e-12 ref (a sum of at most 343 terms 1 / (1 + k), each correctly rounded on
both sides).  They carry over to the averaging: a mean with positive weights that sum to one deviates by no more than the worst of its terms,
plus the rounding of at most 343 additions (343 x 2^-53 = 4e-14 relative).  A voxel is left out of a comparison only where the restatement
itself calls a decision a tie -- with averaging: that of any centre whose patch holds the voxel --, at most 1 % per case, asserted;
tests/test_mppca_box_host.py asserts that on the volumes used here the restatement calls none.

Volumes are 9 x 8 x 7 (mppca_box_numpy.CASES) with four holes in the mask and one isolated voxel: windows clipped on every
side, patches from 1 voxel to 147, fewer and more patch voxels than echoes; two volumes thinner than their window; a 12 x 5 x 4 one for the
seams between the pieces the volume is cut into when the work space is small.

MET2_MPPCA_BOX_PARITY=<path>: the parity cases also write their measured maxima there as JSON (profiles/mppca_box_parity.json is such a file)."""
import ctypes as C
import functools
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mppca_box_numpy as bx                                       # noqa: E402
import mppca_numpy as mp                                           # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID = -1
KEYS = ("out", "sigma", "rank", "n", "wsum")
FIGURES = {}


@pytest.fixture(scope="module")
def motor():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".motor")


def box(data, mask, window, average, work=0, expect=0):
    """met2_mppca_box with every output -> dict of KEYS as numpy (or the return code where `expect` is not 0)"""
    L = importlib.import_module(PKG + "._lib").lib()
    dd = torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64), device="cuda")
    mk = torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device="cuda")
    vol = tuple(dd.shape[:3])
    res = {"out": torch.full_like(dd, -7.0), "sigma": torch.full(vol, -7.0, dtype=torch.float64, device="cuda"),
           "rank": torch.full(vol, -7, dtype=torch.int32, device="cuda"), "n": torch.full(vol, -7, dtype=torch.int32, device="cuda"),
           "wsum": torch.full(vol, -7.0, dtype=torch.float64, device="cuda")}
    rc = L.met2_mppca_box(0, *dd.shape, dd.data_ptr(), mk.data_ptr(), (C.c_int32 * 3)(*window), int(average), int(work),
                          *(res[k].data_ptr() for k in KEYS), None)
    torch.cuda.synchronize()
    assert rc == expect, importlib.import_module(PKG + "._lib").lib().met2_last_error()
    return {k: t.cpu().numpy() for k, t in res.items()} if rc == 0 else rc


def same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def work_bytes(shape, window):
    return importlib.import_module(PKG + ".filters").mppca_work_bytes(shape, window)


@functools.lru_cache(maxsize=None)
def reference(name, average):
    """(data, mask, window, the restatement's result) of a committed case: computed once, shared, never written to"""
    data, mask, window = bx.case(name)
    res = bx.mppca_box(data, mask, window, average=bool(average))
    for a in (data, mask) + tuple(res.values()):
        a.setflags(write=False)
    return data, mask, window, res


# ---- 1. the cube without averaging is met2_mppca

@pytest.mark.parametrize("nt", [3, 32, 63])
@pytest.mark.parametrize("w", [3, 5, 7])
def test_cubic_window_without_averaging_is_met2_mppca_to_the_bit(motor, w, nt):
    data, mask = bx.holed_volume((9, 8, 7), nt, 1)
    out, sigma, rank = motor.mppca_filter(data, mask, window=w, return_maps=True)
    got = box(data, mask, (w, w, w), 0)
    assert np.array_equal(got["out"], out) and np.array_equal(got["sigma"], sigma) and np.array_equal(got["rank"], rank)
    assert (got["n"] >= 2).sum() > 300 and not got["wsum"].any()
    # and through the filter: three equal ints take the box entry
    via = motor.mppca_filter(data, mask, window=(w, w, w), return_maps=True)
    assert all(np.array_equal(a, b) for a, b in zip(via, (out, sigma, rank)))


# ---- 2. parity with the restatement

@pytest.mark.parametrize("average", [0, 1])
@pytest.mark.parametrize("name", ["w331_M3", "w133_M12", "w551_M32", "w357_M33", "w773_M63", "w555_M32", "thin_z", "thin_x"])
def test_parity_with_the_restatement(motor, name, average):
    data, mask, window, ref = reference(name, average)
    got = box(data, mask, window, average)
    off = mask == 0
    assert all(not got[k][off].any() for k in KEYS)
    use = ~ref["tie"] & ~off
    share = float(ref["tie"].sum()) / ref["tie"].size
    scale = np.abs(data).max()
    rs, rw = ref["sigma"][use], ref["wsum"][use]
    fig = {"excluded_share": share, "voxels": int(use.sum()),
           "out": float(np.abs(got["out"][use] - ref["out"][use]).max() / scale),
           "sigma": float(np.max(np.abs(got["sigma"][use] - rs) / np.where(rs > 0, rs, 1.0))),
           "wsum": float(np.max(np.abs(got["wsum"][use] - rw) / np.where(rw > 0, rw, 1.0))),
           "ranks": [int(r) for r in np.unique(got["rank"][use])], "n_patch": [int(ref["n"][use].min()), int(ref["n"][use].max())]}
    print(name, "average" if average else "centre only", fig)
    FIGURES["%s/average=%d" % (name, average)] = fig
    if os.environ.get("MET2_MPPCA_BOX_PARITY"):
        with open(os.environ["MET2_MPPCA_BOX_PARITY"], "w") as f:
            json.dump({"tolerances": {"out": 1e-9, "sigma": 1e-6, "wsum": 1e-12, "excluded_share": 0.01}, "cases": FIGURES}, f, indent=1, sort_keys=True)
    assert share <= 0.01
    assert np.array_equal(got["n"][use], ref["n"][use]) and np.array_equal(got["rank"][use], ref["rank"][use])
    assert fig["out"] <= 1e-9
    assert np.all(np.abs(got["sigma"][use] - rs) <= 1e-6 * rs)
    assert np.all(np.abs(got["wsum"][use] - rw) <= 1e-12 * rw)
    if average:
        assert (got["wsum"][use & (ref["n"] >= 2)] > 0).all()


def test_filter_takes_the_box_window_and_the_average(motor):
    data, mask, window, ref = reference("w551_M32", 1)
    raw = box(data, mask, window, 1)
    out, sigma, rank = motor.mppca_filter(data, mask, window=window, average=True, return_maps=True)
    assert np.array_equal(out, raw["out"]) and np.array_equal(sigma, raw["sigma"]) and np.array_equal(rank, raw["rank"])
    t = motor.mppca_filter(torch.as_tensor(data, device="cuda"), torch.as_tensor(mask, device="cuda"), window=list(window), average=True)
    assert torch.is_tensor(t) and t.is_cuda and np.array_equal(t.cpu().numpy(), out)
    # an int window with the average is the cube
    a = motor.mppca_filter(data, mask, window=3, average=True)
    assert np.array_equal(a, box(data, mask, (3, 3, 3), 1)["out"])
    # every output may be NULL
    L = importlib.import_module(PKG + "._lib").lib()
    dd, mk = torch.as_tensor(data, device="cuda").contiguous(), torch.as_tensor(mask, device="cuda").contiguous()
    o = torch.empty_like(dd)
    for average in (0, 1):
        assert L.met2_mppca_box(0, *dd.shape, dd.data_ptr(), mk.data_ptr(), (C.c_int32 * 3)(*window), average, 0, o.data_ptr(), None, None, None,
                                None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(o.cpu().numpy(), box(data, mask, window, average)["out"])
    with pytest.raises(ValueError, match="window"):
        motor.mppca_filter(data, mask, window=(5, 5, 2))


# ---- 3. the result does not depend on how the volume is cut

def reckoned(c, shape, window):
    """the bytes the library reckons c centres at (include/met2_hip.h, work space): 8 vectors per centre, and never less than one voxel's
    centres at any rank -> (those bytes, the doubles of the pool they leave)"""
    nt = shape[3]
    P = int(np.prod([min(w, n) for w, n in zip(window, shape[:3])]))
    K = min(nt, P)
    pool = max(c * nt * min(K, 8), P * nt * K)
    return 16 + 24 * c + 8 * pool, pool


@pytest.mark.parametrize("name", ["seams", "w551_M32"])
def test_work_space_size_does_not_change_a_bit(motor, name):
    data, mask, window = bx.case(name)
    nx, ny, nz = data.shape[:3]
    lo, dflt = work_bytes(data.shape, window)
    whole = box(data, mask, window, 1)                             # the default holds the whole volume at any rank: one piece
    P = int(np.prod([min(w, n) for w, n in zip(window, data.shape[:3])]))                  # one voxel's centres, at most
    assert lo == reckoned(P, data.shape, window)[0] and dflt > reckoned(nx * ny * nz, data.shape, window)[0]
    again = box(data, mask, window, 1)
    assert same(whole, again)
    planes = reckoned(ny * nz * (window[0] + 2), data.shape, window)[0]            # three planes of output voxels and their halo:
    assert nx >= 9 and lo < planes < reckoned(ny * nz * (window[0] + 3), data.shape, window)[0] < dflt      # at least three pieces along x
    for work in (lo, 2 * lo, planes, dflt - 1):
        assert same(whole, box(data, mask, window, 1, work=work)), work
    assert box(data, mask, window, 1, work=lo - 1, expect=E_INVALID) == E_INVALID
    assert (whole["wsum"][mask != 0] > 0).sum() > 100


def test_a_pool_that_overflows_is_run_again_in_halves(motor):
    # noiseless curves: every patch keeps as many components as it has voxels or echoes (rounding dust passes for signal), far more than the 8
    # per centre the cut is reckoned at.  A work space that holds the whole volume as reckoned then overflows, and its halves, and theirs,
    # run until they fit; whatever the route, the bits are those of the default work space, which holds every centre at any rank.
    shape, window = (9, 8, 7, 32), (5, 5, 1)
    te = 10.0 * np.arange(1, shape[3] + 1)
    g = np.indices(shape[:3]).astype(np.float64)
    t2 = 15.0 + 3.0 * g[0] + 5.0 * g[1] + 7.0 * g[2] + 0.37 * g[0] * g[1] * g[2]
    data = 1000.0 * np.exp(-te / t2[..., None])
    mask = np.ones(shape[:3], dtype=np.uint8)
    mask[3, 3, 3] = 0
    data[3, 3, 3] = 0.0
    whole = box(data, mask, window, 1)
    work, pool = reckoned(int(np.prod(shape[:3])), shape, window)
    assert work < work_bytes(shape, window)[1]
    kept = int(whole["rank"].clip(min=0).sum()) * shape[3]          # the doubles the centres of the whole volume keep
    print("vectors kept: %d doubles, the pool as reckoned: %d" % (kept, pool))
    assert kept > pool                                              # the whole volume overflows (in the restatement it keeps twice the pool)
    assert same(whole, box(data, mask, window, 1, work=work))
    assert same(whole, box(data, mask, window, 1, work=work_bytes(shape, window)[0]))


# ---- 4. the copy-through classes

def test_classes(motor):
    data, mask = bx.holed_volume((9, 8, 7), 12, 1)
    window, p = (3, 5, 3), (4, 3, 3)
    assert mask[p]
    clean = box(data, mask, window, 1)
    iso = (8, 7, 0)                                                # the isolated voxel: copied, rank 1, no vote
    assert clean["n"][iso] == 1 and clean["rank"][iso] == 1 and clean["wsum"][iso] == 0 and clean["sigma"][iso] == 0
    assert np.array_equal(clean["out"][iso], data[iso])
    assert all(not clean[k][mask == 0].any() for k in KEYS) and (mask == 0).sum() > 60
    assert (clean["rank"][mask != 0] >= 0).all()
    bad = np.array(data)
    bad[p + (5,)] = np.nan
    got = box(bad, mask, window, 1)
    g = np.indices(mask.shape)
    dist = [np.abs(g[a] - p[a]) for a in range(3)]
    inside = np.all([dist[a] <= window[a] // 2 for a in range(3)], axis=0) & (mask != 0)
    far = np.any([dist[a] > 2 * (window[a] // 2) for a in range(3)], axis=0)
    assert np.array_equal(got["rank"] == -1, inside) and inside.sum() > 30
    assert np.array_equal(got["out"][p], bad[p], equal_nan=True) and got["wsum"][p] == 0 and got["sigma"][p] == 0
    assert far.sum() > 100 and all(np.array_equal(got[k][far], clean[k][far]) for k in KEYS)
    near = inside & ~far
    near[p] = False
    assert np.isfinite(got["out"][near]).all() and (got["wsum"][near] < clean["wsum"][near]).all()      # fewer votes, none of them poisoned
    # without averaging: the voxels whose patch holds the NaN are copied through
    plain = box(bad, mask, window, 0)
    assert np.array_equal(plain["rank"] == -1, inside) and np.array_equal(plain["out"][inside], bad[inside], equal_nan=True)


# ---- 5. scaling

@pytest.mark.parametrize("average", [0, 1])
@pytest.mark.parametrize("e", [40, -40])
def test_scaling_by_a_power_of_two_is_exact(motor, e, average):
    data, mask, window = bx.case("w357_M33")
    a = box(data, mask, window, average)
    b = box(np.ldexp(data, e), mask, window, average)
    assert np.array_equal(b["out"], np.ldexp(a["out"], e)) and np.array_equal(b["sigma"], np.ldexp(a["sigma"], e))
    assert same(a, b, ("rank", "n", "wsum")) and (a["rank"][mask != 0] > 0).any()


# ---- 6. the drivers

def test_drivers_take_the_window_and_the_average(motor, tmp_path):
    # the drivers' argument lists are fixed, so the two options ride in denoise={'method': 'MPPCA', 'mppca_window': ..., 'mppca_average': ...}
    data, mask, _ = mp.case("driver")
    TE = 10.0 * np.arange(1, data.shape[-1] + 1)
    raw = np.array(data)
    raw[1, 2, 3, 30] = -5.0                                         # clipped before the filter
    prep = np.where(raw * mask[..., None] < 0, 0.0, raw * mask[..., None])
    keys = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param")
    fit = lambda d, **kw: motor.recon_met2_arrays(d, mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0, **kw)

    def pipeline(**filt):
        den, sigma, _ = motor.mppca_filter(prep, mask, return_maps=True, **filt)
        den = np.where(den < 0, 0.0, den)
        return den, sigma, fit(den, prepared=True)

    box_avg = {"method": "MPPCA", "mppca_window": (5, 5, 1), "mppca_average": "yes"}
    den, sigma, want = pipeline(window=(5, 5, 1), average=True)
    got = fit(raw, denoise=box_avg, return_prepared=True)
    assert np.array_equal(got["data_prepared"], den) and np.array_equal(got["MPPCA_sigma"], sigma)
    for k in keys:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert want["MWF"][mask != 0].max() > 0.0
    # the default options are the path of before: met2_mppca with window 5
    den5, sigma5, want5 = pipeline(window=5)
    assert not np.array_equal(den5, den)
    for denoise in ("MPPCA", {"method": "MPPCA"}, {"method": "MPPCA", "mppca_window": 5, "mppca_average": "no"}):
        got5 = fit(raw, denoise=denoise, return_prepared=True)
        assert np.array_equal(got5["data_prepared"], den5) and np.array_equal(got5["MPPCA_sigma"], sigma5)
        for k in keys:
            assert np.array_equal(got5[k], want5[k], equal_nan=True), k
    # rician='direct' takes the noise map of the mode that ran; the device-list leg runs the same filter on devices[0]
    ric = fit(raw, denoise=box_avg, rician="direct")
    assert np.array_equal(ric["sigma"], sigma)
    multi = fit(raw, denoise=box_avg, devices=[0], return_prepared=True)
    assert np.array_equal(multi["data_prepared"], den) and np.array_equal(multi["MWF"], want["MWF"], equal_nan=True)
    # the on-disk driver: Data_denoised.nii.gz and MPPCA_sigma.nii.gz are those of the mode asked for
    nifti = importlib.import_module(PKG + ".nifti")
    nifti.save(nifti.NiftiImage(raw, np.eye(4)), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(mask.astype(np.uint8), np.eye(4)), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/box_"
    motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", box_avg, "brute-force", "no",
                           40.0, 1)
    assert np.array_equal(nifti.load(out + "Data_denoised.nii.gz").get_fdata(), den)
    assert np.array_equal(nifti.load(out + "MPPCA_sigma.nii.gz").get_fdata(), sigma)
    assert np.array_equal(nifti.load(out + "MWF.nii.gz").get_fdata(), want["MWF"], equal_nan=True)
