"""GPU tests of met2_bias_field (csrc/met2_bias.hip), motor.bias_field_filter and bias_correct='yes' in the drivers, against the numpy
restatement of the algorithm (tests/tools/bias_numpy.py, which follows include/met2_hip.h step by step).

Tolerances.  max |field / ref - 1| <= 1e-9, max |out - ref| <= 1e-9 max|v|, the final class parameters within 1e-9 relative: the bar MP-PCA
and Gibbs are pinned at.  tests/test_bias_host.py is what allows it: on these volumes the restatement in fp64 and in long double agree to
1.2e-13, the initial means do not depend on any one sample (so one ulp in a log cannot change them), and one histogram bin in one initial
mean moves the field by far more than 1e-6.

Shapes (bias_numpy.case): three radii, axes shorter than the kernel's half-width and of length 1, a line that crosses a wave and is no
multiple of a tile, radius 0 and 1, holes in the domain and a support that is not the whole volume, 1 and 8 classes, classes at the
variance floor, no outer iteration; tile seams of the smoothing on y and z and three tiles on z (seams), the widest halo, r = 64, across two
seams (r64), 260 chunks of the volume with a support short of it (big) and 260 partials in every second-stage sum (bigall).  Measured on those
four: field 1.6e-14, 3.4e-15, 1.8e-13, and bigall likewise far inside 1e-9 (profiles/bias_parity.json).  The kernels one by one:
tests/test_gpu_bias_stages.py."""
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
import bias_numpy as bn                                            # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
KEYS = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param")


def record(name, figures):
    """with MET2_BIAS_PARITY_JSON set, the measured deviations are kept in that file (profiles/bias_parity.json was written this way)"""
    path = os.environ.get("MET2_BIAS_PARITY_JSON")
    if not path:
        return
    table = json.load(open(path)) if os.path.exists(path) else {}
    table[name] = figures
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def motor():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".motor")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(v, mask, voxel size, kwargs, restatement's result) of a committed case: computed once, shared, never written to"""
    v, mask, vox, kw = bn.case(name)
    res = bn.bias_field(v, mask, vox, **kw)
    for a in (v, mask) + tuple(res.values()):
        if a is not None:                                               # 'bigall' has no mask
            a.setflags(write=False)
    return v, mask, vox, kw, res


@pytest.mark.parametrize("name", bn.CASES)
def test_parity_with_the_restatement(motor, name):
    v, mask, vox, kw, ref = reference(name)
    K = kw.get("n_class", 3)
    out, field, classes = motor.bias_field_filter(v, mask, vox, return_field=True, **kw)
    assert out.dtype == field.dtype == np.float64 and out.shape == field.shape == v.shape and classes.shape == (3 * K,)
    fin = np.isfinite(v)
    e_field = float(np.abs(field / ref["field"] - 1.0).max())
    e_out = float(np.abs(out[fin] - ref["out"][fin]).max() / np.abs(v[fin]).max())
    live = ref["classes"] != 0
    e_cls = float(np.abs(classes[live] / ref["classes"][live] - 1.0).max())
    print("%s %s: max |field / ref - 1| = %.3e, max |out - ref| / max|v| = %.3e, classes %.3e" % (name, v.shape, e_field, e_out, e_cls))
    record(name, {"shape": list(v.shape), "field_rel": e_field, "out_rel_max_v": e_out, "classes_rel": e_cls})
    assert e_field <= 1e-9
    assert e_out <= 1e-9
    assert e_cls <= 1e-9 and np.array_equal(classes[~live], ref["classes"][~live])
    assert np.array_equal(out[~fin], v[~fin], equal_nan=True)           # copied through
    assert np.all(field[~ref["support"]] == 1.0) if kw.get("n_outer", 4) else np.all(field == 1.0)
    if name == "holes":
        assert not ref["support"].all() and np.array_equal(field == 1.0, ref["field"] == 1.0)
    if name in ("coarse", "coarse80", "k8floor"):
        assert (classes[K:2 * K] == 1e-6).any()                         # the variance floor, on the device too
    if name == "outer0":
        assert np.array_equal(out, v)


def test_deterministic_and_independent_of_the_embedding(motor):
    v, mask, vox, kw, ref = reference("phantom")
    a = motor.bias_field_filter(v, mask, vox, return_field=True)
    b = motor.bias_field_filter(v, mask, vox, return_field=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    radii = [bn.radius_weights(20.0, d)[0] for d in vox]
    pad = [(r + 1, r + 3) for r in radii]                                # at least r on every side: Omega and D are the same sets
    big_v = np.pad(v, pad, constant_values=123.0)
    big_m = np.pad(mask, pad, constant_values=0)
    out, field, classes = motor.bias_field_filter(big_v, big_m, vox, return_field=True)
    inner = tuple(slice(p[0], p[0] + n) for p, n in zip(pad, v.shape))
    assert np.array_equal(field[inner], a[1]) and np.array_equal(out[inner], a[0]) and np.array_equal(classes, a[2])
    support = bn.bias_field(big_v, big_m, vox, n_outer=0)["support"]     # reaches r_a into the padding and no further
    assert support[inner].all() and not support.all() and np.all(field[~support] == 1.0)


def test_numpy_and_tensor_faces_and_null_outputs(motor):
    v, mask, vox, kw, ref = reference("wave")
    out, field, classes = motor.bias_field_filter(v, mask, vox, return_field=True)
    plain = motor.bias_field_filter(v, mask, vox)                        # field = classes = NULL
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, out)
    t = motor.bias_field_filter(torch.as_tensor(v, device="cuda"), torch.as_tensor(mask, device="cuda"), vox, return_field=True)
    assert all(torch.is_tensor(x) and x.is_cuda for x in t)
    for x, y in zip(t, (out, field, classes)):
        assert np.array_equal(x.cpu().numpy(), y)
    tp = motor.bias_field_filter(torch.as_tensor(v, device="cuda"), mask, vox)
    assert torch.is_tensor(tp) and np.array_equal(tp.cpu().numpy(), out)
    # one of the two alone, through the C entry
    lib = importlib.import_module(PKG + "._lib")
    import ctypes
    dd = torch.as_tensor(v, device="cuda").contiguous()
    mk = torch.as_tensor(mask, device="cuda").contiguous()
    vx = (ctypes.c_double * 3)(*vox)
    nx, ny, nz = dd.shape
    for want_field, want_classes in ((True, False), (False, True)):
        o = torch.empty_like(dd)
        f = torch.full_like(dd, 99.0)
        c = torch.full((9,), 99.0, dtype=torch.float64, device="cuda")
        assert lib.lib().met2_bias_field(0, nx, ny, nz, dd.data_ptr(), mk.data_ptr(), vx, 3, 4, 10, 20.0, o.data_ptr(),
                                         f.data_ptr() if want_field else None, c.data_ptr() if want_classes else None, None) == 0
        assert np.array_equal(o.cpu().numpy(), out)
        assert np.array_equal(f.cpu().numpy(), field) if want_field else bool((f == 99.0).all())
        assert np.array_equal(c.cpu().numpy(), classes) if want_classes else bool((c == 99.0).all())
    # mask NULL is an all-ones mask
    a = motor.bias_field_filter(v, None, vox, return_field=True)
    b = motor.bias_field_filter(v, np.ones(v.shape, dtype=np.uint8), vox, return_field=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[1], field)
    # the degenerate volumes
    for vol, m, mu in ((v, np.zeros_like(mask), 0.0), (np.full(v.shape, 750.0), mask, np.log(750.0))):
        o, f, c = motor.bias_field_filter(vol, m, vox, return_field=True)
        assert np.array_equal(o, vol) and np.all(f == 1.0)
        assert np.allclose(c[:3], mu, rtol=1e-15, atol=0.0) and np.all(c[3:6] == 0.0) and np.all(c[6:] == 1.0 / 3.0)


def test_return_codes(motor):
    lib = importlib.import_module(PKG + "._lib")
    import ctypes
    L = lib.lib()
    dd = torch.full((8, 8, 8), 5.0, dtype=torch.float64, device="cuda")
    o = torch.full_like(dd, 7.0)

    def call(nx=8, ny=8, nz=8, v=dd, out=o, vox=(2.0, 2.0, 2.0), K=3, n_outer=4, n_em=10, fwhm=20.0):
        return L.met2_bias_field(0, nx, ny, nz, None if v is None else v.data_ptr(), None, None if vox is None else (ctypes.c_double * 3)(*vox),
                                 K, n_outer, n_em, fwhm, None if out is None else out.data_ptr(), None, None, None)

    assert call(v=None) == E_INVALID and call(out=None) == E_INVALID
    assert call(out=dd) == E_INVALID                                   # in place
    assert call(nx=-1) == E_INVALID and call(ny=-1) == E_INVALID and call(nz=-1) == E_INVALID
    assert call(K=0) == E_INVALID and call(n_outer=-1) == E_INVALID and call(n_em=0) == E_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(fwhm=bad) == E_INVALID
        assert call(vox=(bad, 2.0, 2.0)) == E_INVALID and call(vox=(2.0, 2.0, bad)) == E_INVALID
    assert call(vox=None) == E_INVALID
    assert call(K=9) == E_UNSUPPORTED
    assert call(vox=(0.5, 2.0, 2.0)) == E_UNSUPPORTED                  # sigma = 17 voxels: r = 68
    assert call(fwhm=80.0, vox=(2.0, 2.0, 2.0)) == E_UNSUPPORTED
    assert call(nx=2048, ny=1024, nz=1024) == E_UNSUPPORTED            # 2^31 voxels; nothing is read
    for shape in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert call(*shape) == 0
    assert call(0, 8, 8, v=None, out=None) == 0
    assert call(0, 8, 8, K=0) == E_INVALID
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                                      # nothing was launched
    assert call(vox=(0.53, 2.0, 2.0)) == 0                             # r = 64, the widest
    assert call(K=8) == 0 and call(n_outer=0) == 0
    with pytest.raises(lib.Met2Error):
        motor.bias_field_filter(np.ones((4, 4, 4)), n_class=9)
    with pytest.raises(ValueError):
        motor.bias_field_filter(np.ones((4, 4)))
    with pytest.raises(ValueError):
        motor.bias_field_filter(np.ones((4, 4, 4)), np.ones((4, 4, 3)))
    with pytest.raises(ValueError):
        motor.bias_field_filter(np.ones((4, 4, 4)), voxel_size=(1.0, 1.0))


def driver_volume():
    """16 x 16 x 4 x 32: a two-pool decay whose amplitude follows a smooth field, two tissue levels, 1 % noise; the mask leaves a rim out"""
    rng = np.random.default_rng(20261018)
    nx, ny, nz, nt = 16, 16, 4, 32
    TE = 10.0 * np.arange(1, nt + 1)
    x, y, z = np.meshgrid(np.linspace(-1, 1, nx), np.linspace(-1, 1, ny), np.linspace(-1, 1, nz), indexing="ij")
    amp = np.where(x * x + y * y < 0.3, 700.0, 1000.0) * np.exp(0.3 * x - 0.2 * y + 0.1 * z)
    sig = amp[..., None] * (0.15 * np.exp(-TE / 20.0) + 0.85 * np.exp(-TE / 80.0))
    data = sig * (1.0 + 0.01 * rng.standard_normal(sig.shape))
    mask = ((np.abs(x) < 0.9) & (np.abs(y) < 0.9)).astype(np.int64)
    return data, mask, TE


def test_drivers_take_bias_correct(motor, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    data, mask, TE = driver_volume()
    args = (mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    vox = (2.0, 2.5, 4.0)
    plain = motor.recon_met2_arrays(data, *args)
    assert "TWC_bias" not in plain and plain["TWC"][mask != 0].min() > 0.0
    no = motor.recon_met2_arrays(data, *args, bias_correct="no")
    assert sorted(no) == sorted(plain)
    for k in plain:
        assert np.array_equal(no[k], plain[k], equal_nan=True), k
    twc, field, _ = motor.bias_field_filter(plain["TWC"], mask, vox, return_field=True)
    assert np.abs(field - 1.0).max() > 0.05
    for kw in ({}, {"devices": [0]}):
        got = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, **kw)
        assert sorted(got) == sorted(list(plain) + ["TWC_bias"])
        for k in plain:
            if k != "TWC":
                assert np.array_equal(got[k], plain[k], equal_nan=True), (k, kw)
        assert np.array_equal(got["TWC"], twc) and np.array_equal(got["TWC_bias"], field), kw
    with pytest.raises(ValueError, match="voxel_size"):
        motor.recon_met2_arrays(data, *args, bias_correct="yes")
    with pytest.raises(ValueError, match="voxel_size"):
        motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=(1.0, 1.0))
    with pytest.raises(ValueError, match="nx,ny,nz,nt"):
        motor.recon_met2_arrays(data.reshape(-1, 32), mask.reshape(-1), *args[1:], bias_correct="yes", voxel_size=vox)
    with pytest.raises(ValueError, match="bias_correct"):
        motor.recon_met2_arrays(data, *args, bias_correct="maybe", voxel_size=vox)
    with pytest.raises(ValueError, match="distributed"):
        motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, distributed=True)
    # the on-disk driver takes the voxel size from the header
    aff = np.diag([2.0, -2.5, 4.0, 1.0])
    nifti.save(nifti.NiftiImage(data, aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(mask.astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/bc_"
    motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force", "no",
                           40.0, 1, bias_correct="yes")
    for k in KEYS + ("TWC_bias",):
        assert os.path.exists(out + k + ".nii.gz"), k
    assert np.array_equal(nifti.load(out + "TWC.nii.gz").get_fdata(), twc)
    assert np.array_equal(nifti.load(out + "TWC_bias.nii.gz").get_fdata(), field)
    assert np.array_equal(nifti.load(out + "MWF.nii.gz").get_fdata(), plain["MWF"])
    unit = motor.bias_field_filter(plain["TWC"], mask, (1.0, 1.0, 1.0), return_field=True)[1]
    assert np.abs(unit / field - 1.0).max() > 1e-3                     # the header's size was used, not (1, 1, 1)
    with pytest.raises(ValueError, match="bias_correct"):
        motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force",
                               "no", 40.0, 1, bias_correct="maybe")
    assert importlib.import_module(PKG).bias_field_filter is motor.bias_field_filter
