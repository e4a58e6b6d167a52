"""GPU tests of met2_degibbs (csrc/met2_gibbs.hip), motor.gibbs_filter and degibbs='yes' in the drivers, against the numpy restatement of the
algorithm (tests/tools/gibbs_numpy.py: numpy.fft and the selection loop of include/met2_hip.h).

Tolerances.  The shift is a discrete decision; tests/test_gibbs_host.py asserts that on the volumes used here the restatement calls no sample
a tie (margin >= 1e-9 max|slice|, four orders above the 1e-14..1e-13 by which formulations of the shifted lines differ), so no sample is
left out: shift_x and shift_y equal everywhere, |out - ref| <= 1e-9 max|data| (MP-PCA's tolerance; one step of the shift moves a sample by
about 1e-2 of the local gradient, so a wrong shift cannot hide under it).

Shapes: the smallest (8, where the windows reach round the line), odd sizes (no Nyquist bin), lines that cross a wave (65) and the row
tile of the DFT kernels (no multiple of 8), several lines per workgroup (n <= 128) and one (256), the largest against the smallest."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gibbs_numpy as gn                                           # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
KEYS = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param")


@pytest.fixture(scope="module")
def motor():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".motor")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(data, (nsh, minW, maxW), restatement's result) of a committed case: computed once, shared, never written to"""
    data, params = gn.case(name)
    res = gn.degibbs(data, *params)
    for a in (data,) + tuple(res.values()):
        a.setflags(write=False)
    return data, params, res


@pytest.mark.parametrize("name", ["n8", "odd", "mixed", "wave", "long", "extreme", "params", "nsh32"])
def test_parity_with_the_restatement(motor, name):
    data, (nsh, minW, maxW), ref = reference(name)
    assert not gn.ties(ref).any()
    out, sx, sy = motor.gibbs_filter(data, nsh, minW, maxW, return_shifts=True)
    assert out.dtype == np.float64 and sx.dtype == np.int8 and sy.dtype == np.int8 and out.shape == sx.shape == sy.shape == data.shape
    wrong = int((sx != ref["shift_x"]).sum() + (sy != ref["shift_y"]).sum())
    err = np.abs(out - ref["out"]).max() / np.abs(data).max()
    print("%s %s: %d shifts differ, max |out - ref| / max|data| = %.3e, shifts used %d..%d" % (name, data.shape, wrong, err, sx.min(), sx.max()))
    assert np.array_equal(sx, ref["shift_x"])
    assert np.array_equal(sy, ref["shift_y"])
    assert err <= 1e-9
    assert np.abs(sx).max() > 1 and np.abs(sy).max() > 1             # the search does move samples


def test_deterministic_and_slice_by_slice(motor):
    data, (nsh, minW, maxW), _ = reference("mixed")
    a = motor.gibbs_filter(data, return_shifts=True)
    b = motor.gibbs_filter(data, return_shifts=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for z in range(data.shape[2]):
        for e in range(data.shape[3]):
            one = motor.gibbs_filter(np.ascontiguousarray(data[:, :, z:z + 1, e:e + 1]), return_shifts=True)
            for full, part in zip(a, one):
                assert np.array_equal(full[:, :, z, e], part[:, :, 0, 0]), (z, e)


def test_numpy_and_tensor_faces_and_null_shifts(motor):
    data, _, ref = reference("odd")
    out, sx, sy = motor.gibbs_filter(data, return_shifts=True)
    plain = motor.gibbs_filter(data)                                 # shift_x = shift_y = NULL
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, out)
    t = motor.gibbs_filter(torch.as_tensor(data, device="cuda"), return_shifts=True)
    assert all(torch.is_tensor(x) and x.is_cuda for x in t)
    for x, y in zip(t, (out, sx, sy)):
        assert np.array_equal(x.cpu().numpy(), y)
    tp = motor.gibbs_filter(torch.as_tensor(data, device="cuda"))
    assert torch.is_tensor(tp) and np.array_equal(tp.cpu().numpy(), out)
    # one of the two alone
    lib = importlib.import_module(PKG + "._lib")
    dd = torch.as_tensor(data, device="cuda").contiguous()
    o = torch.empty_like(dd)
    s = torch.full(dd.shape, 99, dtype=torch.int8, device="cuda")
    nx, ny, nz, nt = dd.shape
    assert lib.lib().met2_degibbs(0, nx, ny, nz, nt, dd.data_ptr(), 20, 1, 3, o.data_ptr(), None, s.data_ptr(), None) == 0
    assert np.array_equal(o.cpu().numpy(), out) and np.array_equal(s.cpu().numpy(), sy)


def test_non_finite_slice_is_copied_through_and_zero_stays_zero(motor):
    data, _, _ = reference("mixed")
    good = motor.gibbs_filter(data, return_shifts=True)
    bad = np.array(data)
    bad[3, 4, 1, 0] = np.nan
    bad[0, 11, 2, 1] = np.inf
    out, sx, sy = motor.gibbs_filter(bad, return_shifts=True)
    hit = np.zeros(data.shape[2:], dtype=bool)
    hit[1, 0] = hit[2, 1] = True
    assert np.array_equal(out[:, :, hit], bad[:, :, hit], equal_nan=True)
    assert not sx[:, :, hit].any() and not sy[:, :, hit].any()
    for x, y in zip((out, sx, sy), good):
        assert np.array_equal(x[:, :, ~hit], y[:, :, ~hit])
    z, zx, zy = motor.gibbs_filter(np.zeros((16, 12, 2, 1)), return_shifts=True)
    assert not z.any() and not zx.any() and not zy.any()
    mixed = np.array(data)
    mixed[:, :, 0, 0] = 0.0
    assert not motor.gibbs_filter(mixed)[:, :, 0, 0].any()


def test_return_codes(motor):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    dd = torch.zeros((257, 16, 1, 1), dtype=torch.float64, device="cuda")
    o = torch.full_like(dd, 7.0)

    def call(nx=16, ny=16, nz=1, nt=1, nsh=20, minW=1, maxW=3, data=dd, out=o):
        return L.met2_degibbs(0, nx, ny, nz, nt, None if data is None else data.data_ptr(), nsh, minW, maxW,
                              None if out is None else out.data_ptr(), None, None, None)

    assert call(nx=7) == E_UNSUPPORTED
    assert call(nx=257) == E_UNSUPPORTED
    assert call(ny=7) == E_UNSUPPORTED and call(ny=257) == E_UNSUPPORTED
    assert call(nsh=0) == E_INVALID
    assert call(nsh=33) == E_UNSUPPORTED
    assert call(minW=3, maxW=2) == E_INVALID
    assert call(minW=0) == E_INVALID
    assert call(maxW=8) == E_UNSUPPORTED                               # 2 (8 + 1) > 16
    assert call(nx=8, maxW=4) == E_UNSUPPORTED
    assert call(data=None) == E_INVALID and call(out=None) == E_INVALID
    assert call(out=dd) == E_INVALID                                   # in place
    assert call(nx=-1) == E_INVALID
    for shape in ((0, 16, 1, 1), (16, 0, 1, 1), (16, 16, 0, 1), (16, 16, 1, 0)):
        assert call(*shape) == 0
    assert L.met2_degibbs(0, 0, 16, 1, 1, None, 20, 1, 3, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                      # nothing was launched
    assert call(maxW=7) == 0                                           # the widest window that fits 16
    with pytest.raises(lib.Met2Error):
        motor.gibbs_filter(np.zeros((7, 16, 1, 1)))
    with pytest.raises(ValueError):
        motor.gibbs_filter(np.zeros((16, 16, 4)))


def test_drivers_take_degibbs(motor, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    data, mask, TE = gn.driver_volume()
    assert data.shape == (12, 12, 2, 32) and (data < 0).any()
    args = (mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    unrung = motor.gibbs_filter(data)
    assert np.abs(unrung - data).max() > 1.0
    want = motor.recon_met2_arrays(unrung, *args, degibbs="no", return_prepared=True)
    assert want["MWF"][mask != 0].max() > 0.0
    for kw in ({}, {"devices": [0]}):
        got = motor.recon_met2_arrays(data, *args, degibbs="yes", return_prepared=True, **kw)
        for k in KEYS + ("data_prepared",):
            assert np.array_equal(got[k], want[k], equal_nan=True), (k, kw)
    assert np.array_equal(want["data_prepared"], np.maximum(unrung * mask[..., None], 0.0))     # mask and clip come after the filter
    # degibbs='no' is the call without the keyword
    a = motor.recon_met2_arrays(data, *args)
    b = motor.recon_met2_arrays(data, *args, degibbs="no")
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert not np.array_equal(a["MWF"], want["MWF"])
    with pytest.raises(ValueError, match="prepared"):
        motor.recon_met2_arrays(data, *args, prepared=True, degibbs="yes")
    with pytest.raises(ValueError, match="nx,ny,nz,nt"):
        motor.recon_met2_arrays(data.reshape(-1, 32), mask.reshape(-1), *args[1:], degibbs="yes")
    with pytest.raises(ValueError, match="degibbs"):
        motor.recon_met2_arrays(data, *args, degibbs="maybe")
    # the on-disk driver
    aff = np.eye(4)
    nifti.save(nifti.NiftiImage(data, aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(mask.astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/dg_"
    motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force", "no",
                           40.0, 1, degibbs="yes")
    assert np.array_equal(nifti.load(out + "Data_degibbs.nii.gz").get_fdata(), unrung)
    assert np.array_equal(nifti.load(out + "MWF.nii.gz").get_fdata(), want["MWF"])
    for k in KEYS:
        assert os.path.exists(out + k + ".nii.gz"), k
