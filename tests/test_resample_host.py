"""Host-side checks of the affine resampling (no GPU): the restatement the GPU tests compare with (tests/tools/resample_numpy.py) is
scipy.ndimage.affine_transform(mode='constant') and spline_filter(mode='mirror'); its fp64 and long-double legs agree on every input the GPU
tests use; the transform algebra of resample.py (voxel_matrix, invert, from_flirt / to_flirt, one case worked by hand); the wrappers and the
library refuse bad shapes, orders and strides before any device work; motor_atlas_stats writes its tables and the resampled labels."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import resample_numpy as rn                                        # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"


@pytest.fixture(scope="module")
def rs():
    return importlib.import_module(PKG + ".resample")


@pytest.fixture(scope="module")
def motor():
    return importlib.import_module(PKG + ".motor")


def scipy_resample(v, A, shape, order, cval):
    return np.stack([ndimage.affine_transform(x, A[:, :3], offset=A[:, 3], output_shape=shape, order=order, mode="constant", cval=cval) for x in v])


@pytest.mark.parametrize("dims", [(9, 8, 7), (2, 3, 4), (5, 1, 9), (1, 1, 1), (3, 4, 65)])
def test_the_restatement_is_scipys(dims):
    rng = np.random.default_rng(11)
    shape = rn.dst_dims(dims)
    v = rn.volume(rng, dims, 2)
    vmax = np.abs(v).max()
    for name, A in rn.transforms(dims, shape).items():
        for order in (0, 1, 3):
            own, ins = rn.resample(v, A, shape, order, cval=-3.0, return_inside=True)
            ref = scipy_resample(v, A, shape, order, -3.0)
            if order == 0:
                assert np.array_equal(own, ref), (name, order)
            else:
                assert np.abs(own - ref).max() <= 1e-10 * vmax, (name, order)
            assert np.all(own[:, ~ins.astype(bool)] == -3.0) and np.array_equal(ins, rn.inside_map(A, dims, shape))
    ref = np.stack([ndimage.spline_filter(x, order=3, mode="mirror") for x in v])
    assert np.abs(rn.prefilter(v) - ref).max() <= 1e-10 * vmax


def test_the_nearest_neighbour_at_a_half_follows_floor():
    v = np.arange(5.0).reshape(5, 1, 1)
    A = np.column_stack([np.eye(3), [0.5, 0.0, 0.0]])
    got = rn.resample(v, A, (5, 1, 1), 0, cval=-1.0)[:, 0, 0]
    assert got.tolist() == [1.0, 2.0, 3.0, 4.0, -1.0]                  # c = 0.5, 1.5, 2.5, 3.5 -> floor(c + 0.5); 4.5 is outside
    A = np.column_stack([0.5 * np.eye(3), np.zeros(3)])
    assert rn.resample(v, A, (9, 1, 1), 0)[:, 0, 0].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0, 4.0, 4.0]


def test_the_mirror_by_modulo():
    assert rn.mirror(np.arange(-3, 6), 1).tolist() == [0] * 9
    assert rn.mirror(np.arange(-3, 6), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert rn.mirror(np.arange(-3, 6), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert rn.mirror(np.arange(-2, 8), 5).tolist() == [2, 1, 0, 1, 2, 3, 4, 3, 2, 1]


@pytest.mark.parametrize("dims", rn.SRC_DIMS)
def test_fp64_and_long_double_agree_on_the_gpu_tests_inputs(dims):
    rng = np.random.default_rng(sum(dims))
    shape = rn.dst_dims(dims)
    v = rn.volume(rng, dims, max(rn.N_SERIES))
    vmax = np.abs(v).max()
    assert np.abs(rn.prefilter(v) - rn.prefilter(v, np.longdouble)).max() <= 1e-13 * vmax
    for name, A in rn.transforms(dims, shape).items():
        for order in (0, 1, 3):
            a, b = rn.resample(v, A, shape, order, cval=7.0), rn.resample(v, A, shape, order, cval=7.0, dtype=np.longdouble)
            if order == 0:
                assert np.array_equal(a, b)
            else:
                assert np.abs(a - b).max() <= 1e-13 * vmax, (name, order)


def rot(deg, axis):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    m = np.eye(4)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def affine(vox, origin, flip_x=False, deg=0.0):
    a = rot(deg, 2) @ np.diag([-vox[0] if flip_x else vox[0], vox[1], vox[2], 1.0])
    a[:3, 3] = origin
    return a


def test_voxel_matrix_composes_and_inverts(rs):
    src = affine((2.0, 2.0, 3.0), (-90.0, -126.0, -72.0), deg=5.0)
    mid = affine((1.0, 1.5, 1.0), (10.0, -20.0, 30.0), flip_x=True)
    dst = affine((1.5, 1.5, 4.0), (-80.0, 100.0, -60.0), deg=-12.0)
    W = rot(7.0, 0) @ rot(-3.0, 1)
    W[:3, 3] = (4.0, -2.5, 1.0)
    full = lambda A: np.vstack([A, [0, 0, 0, 1.0]])
    # shared scanner space: a voxel of dst and its image in src are the same world point
    A = rs.voxel_matrix(dst, src)
    p = np.array([3.0, 4.0, 5.0, 1.0])
    assert np.allclose(src @ full(A) @ p, dst @ p, rtol=0, atol=1e-10)
    # composition: dst -> mid -> src is dst -> src, and the world matrices multiply in that order
    assert np.allclose(full(rs.voxel_matrix(mid, src)) @ full(rs.voxel_matrix(dst, mid)), full(A), rtol=0, atol=1e-10)
    W2 = rot(2.0, 2)
    assert np.allclose(full(rs.voxel_matrix(mid, src, W)) @ full(rs.voxel_matrix(dst, mid, W2)), full(rs.voxel_matrix(dst, src, W @ W2)), rtol=0, atol=1e-10)
    # inversion: swapping the images and inverting the world matrix inverts A
    assert np.allclose(full(rs.voxel_matrix(src, dst, rs.invert(W))) @ full(rs.voxel_matrix(dst, src, W)), np.eye(4), rtol=0, atol=1e-10)
    assert np.allclose(rs.invert(W) @ W, np.eye(4), rtol=0, atol=1e-14) and np.array_equal(rs.invert(W)[3], [0, 0, 0, 1])
    assert rs.voxel_matrix(dst, src).shape == (3, 4) and rs.voxel_matrix(dst, src).flags.c_contiguous
    assert np.array_equal(rs.voxel_matrix(src, src), np.eye(4)[:3]) or np.allclose(rs.voxel_matrix(src, src), np.eye(4)[:3], rtol=0, atol=1e-13)
    for bad in (np.eye(3), np.zeros((4, 4)), np.full((4, 4), np.nan), np.arange(16.0).reshape(4, 4)):
        with pytest.raises(ValueError):
            rs.voxel_matrix(bad, src)


def test_flirt_round_trip_and_a_case_by_hand(rs):
    W = rot(6.0, 2) @ rot(-4.0, 0)
    W[:3, 3] = (3.0, -7.0, 2.0)
    for flip_src in (False, True):
        for flip_dst in (False, True):
            src = affine((2.0, 2.0, 3.0), (-90.0, -126.0, -72.0), flip_x=flip_src, deg=5.0)
            dst = affine((1.0, 1.5, 1.0), (10.0, -20.0, 30.0), flip_x=flip_dst)
            assert (np.linalg.det(src[:3, :3]) > 0) == (not flip_src)
            M = rs.to_flirt(W, src, (40, 50, 30), dst, (64, 48, 20))
            assert np.allclose(rs.from_flirt(M, src, (40, 50, 30), dst, (64, 48, 20)), W, rtol=0, atol=1e-10)
    # by hand: both images 4 x 4 x 4 at 2 mm with a positive determinant, so FSL counts x from the other end: x_fsl = 2 (3 - i), y_fsl = 2 j.
    # The FLIRT matrix "moving + (2, 3, 0) mm = reference" says 2 (3 - i_ref) = 2 (3 - i_src) + 2, i.e. i_src = i_ref + 1: a world shift of
    # +2 mm along x; and 2 j_ref = 2 j_src + 3: a world shift of -3 mm along y.
    a = np.diag([2.0, 2.0, 2.0, 1.0])
    M = np.eye(4)
    M[:3, 3] = (2.0, 3.0, 0.0)
    want = np.eye(4)
    want[:3, 3] = (2.0, -3.0, 0.0)
    assert np.allclose(rs.from_flirt(M, a, (4, 4, 4), a, (4, 4, 4)), want, rtol=0, atol=1e-14)
    assert np.allclose(rs.voxel_matrix(a, a, want), [[1, 0, 0, 1.0], [0, 1, 0, -1.5], [0, 0, 1, 0]], rtol=0, atol=1e-14)
    # with a negative determinant nothing is flipped: the same matrix is a shift of -2 mm in voxel x = +2 mm in world x (the axis points the other way)
    b = np.diag([-2.0, 2.0, 2.0, 1.0])
    assert np.allclose(rs.from_flirt(M, b, (4, 4, 4), b, (4, 4, 4))[:3, 3], (2.0, -3.0, 0.0), rtol=0, atol=1e-14)
    assert "unpinned" in rs.from_flirt.__doc__


def test_the_wrappers_refuse_before_any_device_work(rs, monkeypatch):
    filters = importlib.import_module(PKG + ".filters")

    def touched(*a, **k):
        raise AssertionError("the device or the library was touched")

    monkeypatch.setattr(rs, "lib", touched)
    monkeypatch.setattr(rs, "_enter", touched)
    A = np.eye(4)[:3]
    v = np.zeros((3, 4, 5))
    for call in (lambda: rs.resample(np.zeros((3, 4)), A, (2, 2, 2)),                       # bad source shapes
                 lambda: rs.resample(np.zeros((2, 3, 4, 5, 6)), A, (2, 2, 2)),
                 lambda: rs.resample(np.zeros((3, 0, 5)), A, (2, 2, 2)),
                 lambda: rs.resample(np.zeros((1, 1, 513)), A, (2, 2, 2)),
                 lambda: rs.resample(np.zeros((0, 3, 4, 5)), A, (2, 2, 2)),
                 lambda: rs.resample(v, A, (2, 2)),                                         # bad destination shapes
                 lambda: rs.resample(v, A, (2, 0, 2)),
                 lambda: rs.resample(v, A, (2048, 2048, 512)),
                 lambda: rs.resample(v, A, (2, 2, 2), order=2),                             # bad orders
                 lambda: rs.resample(v, A, (2, 2, 2), order=-1),
                 lambda: rs.resample(v, A, (2, 2, 2), order="cubic"),
                 lambda: rs.resample(v, A, (2, 2, 2), order=True),
                 lambda: rs.resample(v, np.eye(4), (2, 2, 2)),                              # bad transforms
                 lambda: rs.resample(v, np.full((3, 4), np.inf), (2, 2, 2)),
                 lambda: rs.resample(v, A, (2, 2, 2), layout="echo"),
                 lambda: rs.resample(v, A, (2, 2, 2), order=3, max_work_bytes=-1),
                 lambda: rs.resample_labels(np.zeros((3, 4, 5)), A, (2, 2, 2)),             # float labels
                 lambda: rs.resample_labels(np.zeros((3, 4), dtype=np.int32), A, (2, 2, 2)),
                 lambda: rs.resample_labels(np.zeros((3, 4, 5), dtype=np.int64) + 2 ** 40, A, (2, 2, 2)),
                 lambda: rs.resample_labels(np.zeros((3, 4, 5), dtype=np.int32), A, (2, 2, 2), fill=2 ** 31),
                 lambda: rs.prefilter(np.zeros((3, 4))),
                 lambda: rs.prefilter(np.zeros((3, 4, 600))),
                 lambda: filters.resample_filter(v, A, (2, 2, 2), series_axis=1),
                 lambda: filters.resample_filter(v, A, (2, 2, 2), order=5),
                 lambda: filters.resample_labels_filter(v, A, (2, 2, 2))):
        with pytest.raises(ValueError):
            call()
    # bad strides
    assert rs.layout_strides("series", 8, 100) == (1, 100) and rs.layout_strides("voxel", 8, 100) == (8, 1)
    assert rs.check_strides(8, 100, 1, 100, destination=True) == (1, 100) and rs.check_strides(8, 100, 8, 1, destination=True) == (8, 1)
    assert rs.check_strides(8, 100, 1, 50) == (1, 50)                                       # a source may overlap itself
    for bad in ((0, 1), (1, 0), (-1, 100)):
        with pytest.raises(ValueError, match="positive"):
            rs.check_strides(8, 100, *bad)
    for bad in ((1, 99), (7, 1), (2, 150)):
        with pytest.raises(ValueError, match="share"):
            rs.check_strides(8, 100, *bad, destination=True)


def test_the_library_refuses_before_any_device_work():
    """every refusal of the entries comes before the device is made current: on a machine without one they still answer MET2_E_INVALID (-1) or
    MET2_E_UNSUPPORTED (-2), never MET2_E_HIP; the pointers are never read"""
    _lib = importlib.import_module(PKG + "._lib")
    L = _lib.lib()
    for name in ("met2_resample", "met2_resample_work_bytes", "met2_resample_labels", "met2_resample_prefilter"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    i3 = lambda *d: (C.c_int32 * 3)(*d)
    A = np.ascontiguousarray(np.eye(4)[:3])
    Ap = A.ctypes.data_as(_lib._dp)
    nanA = np.ascontiguousarray(np.full((3, 4), np.nan)).ctypes.data_as(_lib._dp)
    p, q = 4096, 8192                                                 # stand-ins for device pointers: a refused call reads neither

    def resample(order=1, src=(3, 4, 5), S=2, sp=p, svs=1, sss=60, dst=(2, 3, 4), a=Ap, dp=q, dvs=1, dss=24, work=0):
        return L.met2_resample(0, order, i3(*src), S, sp, svs, sss, i3(*dst), a, 0.0, dp, dvs, dss, None, work, None)

    assert resample(order=2) == -1 and resample(order=-1) == -1
    assert resample(src=(3, 0, 5)) == -1 and resample(src=(3, 4, 513)) == -2
    assert resample(dst=(2, 0, 4)) == -1 and resample(dst=(2048, 2048, 512)) == -2
    assert resample(S=0) == -1 and resample(S=32769) == -2
    assert resample(a=nanA) == -1 and resample(a=None) == -1
    assert resample(sp=None) == -1 and resample(dp=None) == -1 and resample(dp=p) == -1
    assert resample(svs=0) == -1 and resample(sss=-60) == -1 and resample(dvs=0) == -1 and resample(dss=0) == -1
    assert resample(dss=23) == -1 and resample(dvs=2, dss=1, S=3) == -1               # two pairs would share an element
    assert resample(order=3, work=-1) == -1 and resample(order=3, work=8 * 60 - 1) == -1
    assert b"480" in L.met2_last_error()
    assert L.met2_resample_labels(0, i3(3, 4, 5), None, i3(2, 2, 2), Ap, 0, q, None, None) == -1
    assert L.met2_resample_labels(0, i3(3, 4, 5), p, i3(2, 2, 2), Ap, 0, p, None, None) == -1
    assert L.met2_resample_labels(0, i3(3, 4, 600), p, i3(2, 2, 2), Ap, 0, q, None, None) == -2
    assert L.met2_resample_labels(0, i3(3, 4, 5), p, i3(2, 2, 2), nanA, 0, q, None, None) == -1
    assert L.met2_resample_prefilter(0, i3(3, 4, 5), 0, p, 1, 60, q, None) == -1
    assert L.met2_resample_prefilter(0, i3(3, 4, 5), 2, p, 0, 60, q, None) == -1
    assert L.met2_resample_prefilter(0, i3(3, 4, 5), 2, p, 1, 60, p, None) == -1
    assert L.met2_resample_prefilter(0, i3(0, 4, 5), 2, p, 1, 60, q, None) == -1


def test_work_bytes(rs):
    assert rs.work_bytes(0, (9, 8, 7), 8) == (0, 0) and rs.work_bytes(1, (9, 8, 7), 8) == (0, 0)
    assert rs.work_bytes(3, (9, 8, 7), 8) == (8 * 504, 8 * 8 * 504) and rs.work_bytes(3, (9, 8, 7)) == (8 * 504, 8 * 504)
    assert rs.work_bytes(3, (512, 512, 512), 32) == (2 ** 30, 2 ** 30)                 # the cap never goes below one series
    assert rs.work_bytes(3, (128, 128, 64), 32768) == (2 ** 23, 2 ** 30)
    with pytest.raises(ValueError):
        rs.work_bytes(2, (9, 8, 7))
    assert (rs.MAX_AXIS, rs.MAX_SERIES) == (512, 32768)
    text = open(os.path.join(ROOT, "include", "met2_hip.h")).read()
    assert "#define MET2_RESAMPLE_MAX_AXIS 512" in text and "#define MET2_RESAMPLE_MAX_SERIES 32768" in text


def test_motor_atlas_stats_writes_its_tables(motor, monkeypatch, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    filters = importlib.import_module(PKG + ".filters")
    assert motor.resample_filter is filters.resample_filter and motor.resample_labels_filter is filters.resample_labels_filter
    assert motor.atlas_stats_filter is filters.atlas_stats_filter
    rng = np.random.default_rng(5)
    shape, n_t2 = (4, 5, 3), 6
    aff = affine((2.0, 2.0, 3.0), (-10.0, 5.0, 0.0))
    out = str(tmp_path) + os.sep
    maps = {k: rng.random(shape) for k in motor.STAT_QUANTITIES}
    maps["fsol_4D"] = rng.random(shape + (n_t2,))
    for k, a in maps.items():
        nifti.save(nifti.NiftiImage(a, aff), out + k + ".nii.gz")
    lab_aff = affine((1.0, 1.0, 1.5), (-12.0, 4.0, -1.0), deg=4.0)
    atlas = rng.integers(0, 4, (8, 10, 6)).astype(np.int16)
    nifti.save(nifti.NiftiImage(atlas, lab_aff), out + "atlas.nii.gz")
    W = rot(3.0, 1)
    np.savetxt(out + "world.txt", W)
    seen = {}

    def canned(L, q):
        return {"n": rng.integers(1, 9, (L, 8)).astype(np.float64), "mean": rng.standard_normal((L, 8)), "std": rng.random((L, 8)),
                "quantiles": rng.standard_normal((L, 8, len(q))), "spectrum_mean": rng.random((L, n_t2)),
                "spectrum_quantiles": rng.random((L, n_t2, len(q)))}

    def fake_atlas(res, labels, labels_affine, affine_, world=None, q=None, device=0):
        seen.update(res=res, labels=labels, labels_affine=labels_affine, affine=affine_, world=world)
        st = dict(canned(2, (0.025, 0.25, 0.5, 0.75, 0.975)), labels=np.array([1, 3]), quantities=motor.STAT_QUANTITIES,
                  q=np.array([0.025, 0.25, 0.5, 0.75, 0.975]), T2s=res["T2s"])
        st["labels_resampled"] = (np.arange(np.prod(shape)).reshape(shape) % 4).astype(np.int32)
        return st

    def fake_label_stats(res, labels, q=None, device=0):
        seen["whole"] = np.asarray(labels)
        return canned(1, q)

    monkeypatch.setattr(motor, "atlas_stats_filter", fake_atlas)
    monkeypatch.setattr(motor, "label_stats_filter", fake_label_stats)
    st = motor.motor_atlas_stats(out, out + "atlas.nii.gz", out + "world.txt", names={1: "CC", 2: "unused"})
    # what reached the device call: the maps as written, the atlas with its affine, the world matrix
    for k in maps:
        assert np.array_equal(seen["res"][k], maps[k])
    assert np.allclose(seen["res"]["T2s"], np.logspace(1, np.log10(2000.0), n_t2))
    assert np.array_equal(seen["labels"], atlas) and seen["labels"].dtype.kind == "i"
    assert np.allclose(seen["labels_affine"], lab_aff, atol=1e-5) and np.allclose(seen["affine"], aff, atol=1e-5) and np.allclose(seen["world"], W)
    assert np.array_equal(seen["whole"], (st["labels_resampled"] > 0).astype(np.int32))
    # the files
    back = nifti.load(out + "ROIs_resampled.nii.gz")
    assert np.array_equal(back.get_fdata(), st["labels_resampled"]) and np.allclose(back.affine, aff, atol=1e-5)
    rows = [line.split(",") for line in open(out + "table_roi_stats.csv").read().split()]
    assert [r[0] for r in rows] == ["CC"] * 8 + ["3"] * 8 + ["all"] * 8 and [r[1] for r in rows] == list(motor.STAT_QUANTITIES) * 3
    num = np.array([[float(x) for x in r[2:]] for r in rows])
    for i in range(3):
        src = st["all"] if i == 2 else {k: st[k][i] for k in motor.STAT_KEYS}
        assert np.array_equal(num[8 * i:8 * i + 8], np.column_stack([src["n"], src["mean"], src["std"], src["quantiles"]]))
    spectra = np.loadtxt(out + "table_roi_spectra.csv", delimiter=",")
    assert np.array_equal(spectra, np.vstack([st["T2s"], st["spectrum_mean"], st["all"]["spectrum_mean"][None]]))
    # without a world matrix the images share scanner space; a label image that is not 3-D integers is refused
    motor.motor_atlas_stats(out, out + "atlas.nii.gz")
    assert seen["world"] is None
    nifti.save(nifti.NiftiImage(atlas + 0.5, lab_aff), out + "bad.nii.gz")
    with pytest.raises(ValueError, match="integers"):
        motor.motor_atlas_stats(out, out + "bad.nii.gz")
