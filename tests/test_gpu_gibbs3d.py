"""GPU tests of met2_degibbs3d and met2_gibbs_split3d (csrc/met2_gibbs.hip), motor.gibbs_filter(mode='3d'), gibbs.gibbs_split3d and
degibbs='3d' in the drivers, against the numpy restatement of the algorithm (tests/tools/gibbs3d_numpy.py: numpy.fft.fftn and gibbs_numpy's
operator U).

Tolerances.  The shift is a discrete decision; tests/test_gibbs3d_host.py asserts that on the noise volumes used here the restatement calls
no sample a tie (margin >= 1e-9 max|echo volume|), so no sample is left out: the three shift maps equal everywhere and
|out - ref| <= 1e-9 max|echo volume|, echo by echo (the tolerance tests/test_gpu_gibbs.py holds the 2-D filter to).  The ball phantom has
flat regions and so a few ties (0.01 % of the choices): there the shifts are compared off the restatement's ties.  The split is held to
1e-12 max|V| (the bound of the stage tests of the 2-D filter).

Shapes (gibbs3d_numpy.CASES): the smallest (8 along all axes), odd sizes, one, two and three even axes (the rule for the Nyquist lines),
each axis at 255 / 256 or across a step of the line kernel's 256 / n lines per workgroup (128 | 129, 85 | 86), z lines one below, at and
above the tile of 8 of the DFT passes (15, 16, 17), cubes, more echoes than the gather's tile of 32, and one echo more than a chunk holds
(echoes are independent, so the reference of the large volume is the GPU's own result on its 37 distinct echoes, which the parity test
pins to numpy)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gibbs_numpy as gn                                           # noqa: E402
import gibbs3d_numpy as g3                                         # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
KEYS = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param")
SHIFTS = ("shift_x", "shift_y", "shift_z")


@pytest.fixture(scope="module")
def motor():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".motor")


@pytest.fixture(scope="module")
def gibbs(motor):
    return importlib.import_module(PKG + ".gibbs")


def echo_error(out, want, data):
    """max over the echoes of max |out - want| / max|echo volume| (1 for an all-zero echo)"""
    scale = np.abs(data).max(axis=(0, 1, 2), keepdims=True)
    scale = np.where(scale > 0, scale, 1.0)
    return float((np.abs(out - want) / scale).max())


@pytest.mark.parametrize("name", sorted(g3.CASES))
def test_parity_with_the_restatement(motor, name):
    data, params, ref = g3.reference(name)
    nsh, minW, maxW = params
    assert not g3.ties(ref).any()
    got = motor.gibbs_filter(data, nsh, minW, maxW, return_shifts=True, mode="3d")
    assert len(got) == 4 and got[0].dtype == np.float64 and all(s.dtype == np.int8 for s in got[1:])
    assert all(g.shape == data.shape for g in got)
    wrong = int(sum((s != ref[k]).sum() for s, k in zip(got[1:], SHIFTS)))
    err = echo_error(got[0], ref["out"], data)
    margin = g3.min_margin(ref)
    print("%s %s: %d shifts differ, max per echo |out - ref| / max|echo| = %.3e, smallest margin %.2e" % (name, data.shape, wrong, err, margin))
    g3.record("parity/" + name, {"shape": list(data.shape), "params": list(params), "out": err, "wrong_shifts": wrong, "min_margin": margin})
    for s, k in zip(got[1:], SHIFTS):
        assert np.array_equal(s, ref[k]), k
        assert np.abs(s).max() >= min(2, nsh), k                   # the search does move samples, along every axis
    assert err <= 1e-9


def test_ball(motor):
    img, truth, flat = g3.ball_phantom()
    ref = g3.ball_reference()
    data = np.ascontiguousarray(img[..., None])
    out, sx, sy, sz = motor.gibbs_filter(data, return_shifts=True, mode="3d")
    tie = [ref["margin_" + a] < g3.TIE for a in g3.AXES]
    share = float(sum(t.sum() for t in tie)) / (3 * img.size)
    any_tie = tie[0] | tie[1] | tie[2]
    wrong = [int(((s != ref[k]) & ~t).sum()) for s, k, t in zip((sx, sy, sz), SHIFTS, tie)]
    err = float(np.abs(out - ref["out"])[~any_tie].max() / np.abs(img).max())
    two = motor.gibbs_filter(data)[..., 0]
    e0, e2, e3 = g3.rms(img, truth, flat), g3.rms(two, truth, flat), g3.rms(out[..., 0], truth, flat)
    print("ball: ties %.4f %% of the choices, shifts that differ off them %s, |out - ref| / max|V| off them %.3e; rms error input %.3f, "
          "2-D %.3f, 3-D %.3f (ratios %.2f, %.2f)" % (100 * share, wrong, err, e0, e2, e3, e3 / e0, e3 / e2))
    g3.record("ball", {"tie_share": share, "wrong_shifts_off_ties": wrong, "out_off_ties": err, "rms_input": e0, "rms_2d": e2, "rms_3d": e3,
                       "min_margin": g3.min_margin(ref)})
    assert share <= 1e-3
    assert wrong == [0, 0, 0]
    assert err <= 1e-9
    assert e3 <= 0.5 * e0
    assert e3 <= 0.75 * e2


@pytest.mark.parametrize("name", ["n8", "odd", "mixed", "zlpb2", "zwave", "ztile17", "cube33"])     # three even axes, none, three, two, one, two, none
def test_split3d(gibbs, name):
    data, _, ref = g3.reference(name)
    parts = gibbs.gibbs_split3d(data)
    scale = np.abs(data).max(axis=(0, 1, 2), keepdims=True)
    dev = [float((np.abs(p - ref[k]) / scale).max()) for p, k in zip(parts, ("ix", "iy", "iz"))]
    total = float((np.abs(parts[0] + parts[1] + parts[2] - data) / scale).max())
    print("%s %s: parts against the restatement %s, |Ix + Iy + Iz - V| %.2e, of max|V|" % (name, data.shape, ["%.2e" % d for d in dev], total))
    g3.record("split/" + name, {"shape": list(data.shape), "parts": dev, "sum": total})
    assert max(dev) <= 1e-12
    assert total <= 1e-12
    t = gibbs.gibbs_split3d(torch.as_tensor(data, device="cuda"))
    assert all(torch.is_tensor(x) and x.is_cuda for x in t)
    for x, y in zip(t, parts):
        assert np.array_equal(x.cpu().numpy(), y)


def test_chunk_seam(motor):
    """8 x 8 x 8 x 8193: a chunk holds 2^22 / 512 = 8192 echoes, the second chunk one.  Then non-finite echoes either side of the seam and at
    the edges of the gather's tiles of 32 echoes."""
    small, _, _ = g3.reference("echoes37")
    period, nt = small.shape[3], (1 << 22) // 512 + 1
    big = np.ascontiguousarray(small[..., np.arange(nt) % period])
    want = motor.gibbs_filter(small, return_shifts=True, mode="3d")
    got = motor.gibbs_filter(big, return_shifts=True, mode="3d")

    def differing(got, pick):
        bad = np.zeros(pick.size, dtype=bool)
        for g, w in zip(got, want):
            bad |= (g[..., pick] != w[..., pick % period]).any(axis=(0, 1, 2))
        return pick[bad]

    assert differing(got, np.arange(nt)).size == 0
    bad = big.copy()
    hit = [0, 31, 32, nt - 2, nt - 1]                                 # nt - 2 is the last echo of the first chunk, nt - 1 the second chunk
    for k, e in enumerate(hit):
        bad[k % 8, (3 * k) % 8, (5 * k) % 8, e] = (np.nan, np.inf, -np.inf)[k % 3]
    out, sx, sy, sz = motor.gibbs_filter(bad, return_shifts=True, mode="3d")
    assert np.array_equal(out[..., hit], bad[..., hit], equal_nan=True)                          # unchanged
    assert not sx[..., hit].any() and not sy[..., hit].any() and not sz[..., hit].any()
    clean = np.setdiff1d(np.arange(nt), hit)
    assert {1, 30, 33, nt - 3} <= set(clean.tolist())
    assert differing((out, sx, sy, sz), clean).size == 0


def test_deterministic_and_echo_by_echo(motor):
    data, _, _ = g3.reference("mixed")
    a = motor.gibbs_filter(data, return_shifts=True, mode="3d")
    b = motor.gibbs_filter(data, return_shifts=True, mode="3d")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for e in range(data.shape[3]):
        one = motor.gibbs_filter(np.ascontiguousarray(data[..., e:e + 1]), return_shifts=True, mode="3d")
        for full, part in zip(a, one):
            assert np.array_equal(full[..., e], part[..., 0]), e


def test_faces_null_shifts_and_the_2d_mode(motor):
    data, _, _ = g3.reference("odd")
    out, sx, sy, sz = motor.gibbs_filter(data, return_shifts=True, mode="3d")
    plain = motor.gibbs_filter(data, mode="3d")                      # the three shift maps NULL
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, out)
    t = motor.gibbs_filter(torch.as_tensor(data, device="cuda"), return_shifts=True, mode="3d")
    assert len(t) == 4 and all(torch.is_tensor(x) and x.is_cuda for x in t)
    for x, y in zip(t, (out, sx, sy, sz)):
        assert np.array_equal(x.cpu().numpy(), y)
    tp = motor.gibbs_filter(torch.as_tensor(data, device="cuda"), mode="3d")
    assert torch.is_tensor(tp) and np.array_equal(tp.cpu().numpy(), out)
    # one of the three alone
    lib = importlib.import_module(PKG + "._lib")
    dd = torch.as_tensor(data, device="cuda").contiguous()
    o = torch.empty_like(dd)
    s = torch.full(dd.shape, 99, dtype=torch.int8, device="cuda")
    nx, ny, nz, nt = dd.shape
    assert lib.lib().met2_degibbs3d(0, nx, ny, nz, nt, dd.data_ptr(), 20, 1, 3, o.data_ptr(), None, None, s.data_ptr(), None) == 0
    assert np.array_equal(o.cpu().numpy(), out) and np.array_equal(s.cpu().numpy(), sz)
    # mode='2d' is the default call, and another filter than '3d'
    d2 = motor.gibbs_filter(data, return_shifts=True)
    m2 = motor.gibbs_filter(data, return_shifts=True, mode="2d")
    assert len(d2) == len(m2) == 3
    for x, y in zip(d2, m2):
        assert np.array_equal(x, y)
    assert not np.array_equal(d2[0], out)
    with pytest.raises(ValueError, match="mode"):
        motor.gibbs_filter(data, mode="4d")


def test_on_a_side_stream_after_a_producer_kernel(motor):
    """the filter on a tensor that a kernel just enqueued on a non-default stream is still writing, under that stream"""
    data, _, _ = g3.reference("mixed")
    base = torch.as_tensor(data, device="cuda")
    want = motor.gibbs_filter(base * 2.0 + 1.0, return_shifts=True, mode="3d")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(1 << 24, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big * 1.0000001                                    # work ahead of the producer on the same stream
        made = base * 2.0 + 1.0
        got = motor.gibbs_filter(made, return_shifts=True, mode="3d")
    side.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_return_codes(motor, gibbs):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    dd = torch.zeros((16, 16, 257, 1), dtype=torch.float64, device="cuda")
    o = torch.full_like(dd, 7.0)
    o2, o3 = torch.full_like(dd, 7.0), torch.full_like(dd, 7.0)
    ptr = lambda t: None if t is None else t.data_ptr()

    def call(nx=16, ny=16, nz=16, nt=1, nsh=20, minW=1, maxW=3, data=dd, out=o):
        return L.met2_degibbs3d(0, nx, ny, nz, nt, ptr(data), nsh, minW, maxW, ptr(out), None, None, None, None)

    def split(nx=16, ny=16, nz=16, nt=1, data=dd, ix=o, iy=o2, iz=o3):
        return L.met2_gibbs_split3d(0, nx, ny, nz, nt, ptr(data), ptr(ix), ptr(iy), ptr(iz), None)

    for f in (call, split):
        assert f(nz=7) == E_UNSUPPORTED and f(nz=257) == E_UNSUPPORTED
        assert f(nx=7) == E_UNSUPPORTED and f(nx=257) == E_UNSUPPORTED
        assert f(ny=7) == E_UNSUPPORTED and f(ny=257) == E_UNSUPPORTED
        assert f(data=None) == E_INVALID
        assert f(nz=-1) == E_INVALID
        for shape in ((0, 16, 16, 1), (16, 0, 16, 1), (16, 16, 0, 1), (16, 16, 16, 0)):
            assert f(*shape) == 0
    assert call(nz=8, maxW=4) == E_UNSUPPORTED                         # 2 (4 + 1) > 8
    assert call(maxW=8) == E_UNSUPPORTED
    assert call(nsh=0) == E_INVALID and call(nsh=33) == E_UNSUPPORTED
    assert call(minW=3, maxW=2) == E_INVALID and call(minW=0) == E_INVALID
    assert call(out=None) == E_INVALID
    assert call(out=dd) == E_INVALID                                   # in place
    assert split(ix=None) == E_INVALID and split(iy=None) == E_INVALID and split(iz=None) == E_INVALID
    assert split(ix=dd) == E_INVALID and split(iy=o) == E_INVALID and split(iz=o2) == E_INVALID
    assert L.met2_degibbs3d(0, 16, 16, 0, 1, None, 20, 1, 3, None, None, None, None, None) == 0
    assert call(nz=0, nsh=33) == E_UNSUPPORTED                         # the parameter checks come first
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((o2 == 7.0).all()) and bool((o3 == 7.0).all())       # nothing was launched
    assert call(maxW=7) == 0                                           # the widest window that fits 16
    with pytest.raises(lib.Met2Error):
        motor.gibbs_filter(np.zeros((16, 16, 7, 1)), mode="3d")
    with pytest.raises(lib.Met2Error):
        gibbs.gibbs_split3d(np.zeros((16, 16, 7, 1)))
    with pytest.raises(ValueError):
        motor.gibbs_filter(np.zeros((16, 16, 16)), mode="3d")


def test_drivers_take_degibbs_3d(motor, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    data, mask, TE = g3.driver_volume3d()
    assert data.shape == (12, 12, 8, 32)
    args = (mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    unrung = motor.gibbs_filter(data, mode="3d")
    want = motor.recon_met2_arrays(unrung, *args, degibbs="no", return_prepared=True)
    assert want["MWF"][mask != 0].max() > 0.0
    for kw in ({}, {"devices": [0]}):
        got = motor.recon_met2_arrays(data, *args, degibbs="3d", return_prepared=True, **kw)
        for k in KEYS + ("data_prepared",):
            assert np.array_equal(got[k], want[k], equal_nan=True), (k, kw)
    assert np.array_equal(want["data_prepared"], np.maximum(unrung * mask[..., None], 0.0))     # mask and clip come after the filter
    yes = motor.recon_met2_arrays(data, *args, degibbs="yes")
    for k in KEYS:
        assert not np.array_equal(yes[k], want[k], equal_nan=True), k
    with pytest.raises(ValueError, match="prepared"):
        motor.recon_met2_arrays(data, *args, prepared=True, degibbs="3d")
    with pytest.raises(ValueError, match="nx,ny,nz,nt"):
        motor.recon_met2_arrays(data.reshape(-1, 32), mask.reshape(-1), *args[1:], degibbs="3d")
    with pytest.raises(ValueError, match="degibbs"):
        motor.recon_met2_arrays(data, *args, degibbs="3D")
    # the on-disk drivers
    aff = np.eye(4)
    rois = np.zeros(mask.shape, dtype=np.uint8)
    rois[2:6, 2:6, 2:6] = 1
    rois[6:10, 6:10, 2:6] = 2
    for name, vol in (("data", data), ("mask", mask.astype(np.uint8)), ("rois", rois)):
        nifti.save(nifti.NiftiImage(vol, aff), str(tmp_path / (name + ".nii.gz")))
    out = str(tmp_path) + "/dg_"
    motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force", "no",
                           40.0, 1, degibbs="3d")
    assert np.array_equal(nifti.load(out + "Data_degibbs.nii.gz").get_fdata(), unrung)
    assert np.array_equal(nifti.load(out + "MWF.nii.gz").get_fdata(), want["MWF"])
    roi = []
    for mode in ("3d", "yes"):
        d = str(tmp_path) + "/roi_%s_" % mode
        roi.append(motor.motor_recon_met2_ROIs(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), str(tmp_path / "rois.nii.gz"), d,
                                               3000.0, "L2", "None", "brute-force", "no", 40.0, 1, degibbs=mode))
    assert len(roi[0]["MWF"]) == 2 and not np.array_equal(roi[0]["fsol"], roi[1]["fsol"])
