"""The affine resampling on the device (met2_resample, met2_resample_labels, met2_resample_prefilter; include/met2_hip.h states the contract)
against its numpy restatement (tests/tools/resample_numpy.py, which tests/test_resample_host.py holds against scipy): the inside map, order 0
and the labels equal in every voxel -- the coordinates are reproducible to the bit, so no voxel is set aside as a tie --; orders 1 and 3 and
the prefilter stage within 1e-12 max|src| of the long-double restatement (the project's stage-test bound; the fp64 restatement itself lies at
at most 1e-14 of it).  Source dims: axes shorter than the cubic support, the wave width along the z-line tile and one tile plus one; every
transform in both layouts with 1, 3, 8 and 9 series (9 series voxel-major: a group of 16 lanes per voxel, 8: of 8, 3 and 1: one thread per voxel).
Measured on an MI355X (profiles/resample_parity.json): order 1 2.5e-16, order 3 1.6e-15, prefilter 8.3e-15, each relative to max|src|.
With MET2_RESAMPLE_PARITY_OUT=<file> the module writes its measured maxima there as JSON."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import resample_numpy as rn                                        # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
BOUND = 1e-12
CVAL = -7.5
MAXIMA = {"order1": 0.0, "order3": 0.0, "prefilter": 0.0}


@pytest.fixture(scope="module")
def rs():
    yield importlib.import_module(PKG + ".resample")
    path = os.environ.get("MET2_RESAMPLE_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"bound": BOUND, "relative_to": "max|src| = 100", "max_abs_error_over_max_src": MAXIMA}, f, indent=1)


@pytest.fixture(scope="module")
def motor():
    return importlib.import_module(PKG + ".motor")


_REF = {}


def reference(dims):
    """the inputs and the restatement's results of one source grid, computed once: (v [9, ...], {(transform, order): (ref long double, inside)})"""
    if dims not in _REF:
        rng = np.random.default_rng(sum(dims))
        shape = rn.dst_dims(dims)
        v = rn.volume(rng, dims, max(rn.N_SERIES))
        refs = {}
        for name, A in rn.transforms(dims, shape).items():
            for order in (0, 1, 3):
                refs[name, order] = rn.resample(v, A, shape, order, cval=CVAL, dtype=np.longdouble, return_inside=True)
        _REF[dims] = (v, refs)
    return _REF[dims]


def to_layout(v, layout):
    return np.ascontiguousarray(v if layout == "series" else np.moveaxis(v, 0, -1))


def from_layout(a, layout):
    return a if layout == "series" else np.moveaxis(a, -1, 0)


def note(key, err, vmax):
    MAXIMA[key] = max(MAXIMA[key], float(err / vmax))


@pytest.mark.parametrize("dims", rn.SRC_DIMS)
def test_every_transform_layout_and_series_count(rs, dims):
    v, refs = reference(dims)
    shape = rn.dst_dims(dims)
    vmax = np.abs(v).max()
    for name, A in rn.transforms(dims, shape).items():
        for layout in ("series", "voxel"):
            for S in rn.N_SERIES:
                src = to_layout(v[:S], layout)
                for order in (0, 1, 3):
                    got, ins = rs.resample(src, A, shape, order=order, cval=CVAL, layout=layout, return_inside=True)
                    got = from_layout(got, layout)
                    ref, ref_ins = refs[name, order]
                    where = (dims, name, layout, S, order)
                    assert np.array_equal(ins, ref_ins), where
                    if order == 0:
                        assert np.array_equal(got, ref[:S]), where
                        continue
                    err = np.abs(got - ref[:S]).max()
                    note("order%d" % order, err, vmax)
                    print("%s max error %.3e" % (where, err))
                    assert err <= BOUND * vmax, where
                    exact = name in ("identity", "shift", "flip") and order == 1
                    if exact:                                       # integer coordinates: weights 1 and 0, the sample itself
                        assert np.array_equal(got, rn.resample(v[:S], A, shape, 0, cval=CVAL)), where


def test_the_exact_cases_by_construction(rs):
    """identity, integer shift and flip stated without the restatement; a point exactly on c = 0 and on c = n - 1 is inside"""
    dims = (9, 8, 7)
    v, _ = reference(dims)
    v = v[:3]
    eye = np.column_stack([np.eye(3), np.zeros(3)])
    for order in (0, 1):
        got, ins = rs.resample(v, eye, dims, order=order, cval=CVAL, return_inside=True)
        assert np.array_equal(got, v) and ins.all()
        shift = np.column_stack([np.eye(3), [2.0, -1.0, 3.0]])
        got, ins = rs.resample(v, shift, dims, order=order, cval=CVAL, return_inside=True)
        want = np.full_like(v, CVAL)
        want[:, :7, 1:, :4] = v[:, 2:, :7, 3:]
        assert np.array_equal(got, want) and np.array_equal(ins.astype(bool), want[0] != CVAL)
        for axis in range(3):
            flip = np.column_stack([np.eye(3), np.zeros(3)])
            flip[axis, axis], flip[axis, 3] = -1.0, dims[axis] - 1.0
            got, ins = rs.resample(v, flip, dims, order=order, cval=CVAL, return_inside=True)
            assert np.array_equal(got, np.flip(v, axis=1 + axis)) and ins.all()       # the end voxels sit exactly on c = n - 1 and c = 0
    got = rs.resample(v, eye, dims, order=3)
    assert np.abs(got - v).max() <= BOUND * np.abs(v).max()
    # nearest neighbour at c = x.5 follows floor(c + 0.5), on the device as in the restatement
    line = np.arange(5.0).reshape(5, 1, 1)
    half = np.column_stack([np.eye(3), [0.5, 0.0, 0.0]])
    assert rs.resample(line, half, (5, 1, 1), order=0, cval=-1.0)[:, 0, 0].tolist() == [1.0, 2.0, 3.0, 4.0, -1.0]
    scale = np.column_stack([0.5 * np.eye(3), np.zeros(3)])
    assert rs.resample(line, scale, (9, 1, 1), order=0)[:, 0, 0].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0, 4.0, 4.0]


@pytest.mark.parametrize("dims", rn.SRC_DIMS)
def test_the_prefilter_stage(rs, dims):
    v, _ = reference(dims)
    vmax = np.abs(v).max()
    ref = rn.prefilter(v, np.longdouble)
    for layout in ("series", "voxel"):
        for S in rn.N_SERIES:
            got = rs.prefilter(to_layout(v[:S], layout), layout=layout)
            err = np.abs(got - ref[:S]).max()
            note("prefilter", err, vmax)
            print("%s prefilter max error %.3e" % ((dims, layout, S), err))
            assert got.shape == (S,) + dims and err <= BOUND * vmax, (dims, layout, S)
    assert np.array_equal(rs.prefilter(v[0]), rs.prefilter(v[:1])[0])


@pytest.mark.parametrize("dims", rn.SRC_DIMS)
def test_labels(rs, dims):
    rng = np.random.default_rng(3)
    lab = rng.integers(-2, 2000, dims).astype(np.int32)
    shape = rn.dst_dims(dims)
    for name, A in rn.transforms(dims, shape).items():
        got, ins = rs.resample_labels(lab, A, shape, fill=-9, return_inside=True)
        assert got.dtype == np.int32 and np.array_equal(got, rn.resample_labels(lab, A, shape, fill=-9)), (dims, name)
        assert np.array_equal(ins, rn.inside_map(A, dims, shape)), (dims, name)
    dev = torch.as_tensor(lab.astype(np.int64), device="cuda")
    out = rs.resample_labels(dev, A, shape, fill=-9)
    assert torch.is_tensor(out) and out.is_cuda and out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), got)


def test_the_bits_do_not_depend_on_chunking_run_or_stacking(rs):
    dims, S = (9, 8, 7), 9
    shape = rn.dst_dims(dims)
    v, _ = reference(dims)
    A = rn.transforms(dims, shape)["rotated"]
    lo, dflt = rs.work_bytes(3, dims, S)
    assert (lo, dflt) == (8 * 504, 9 * 8 * 504)
    for layout in ("series", "voxel"):
        src = to_layout(v, layout)
        for order in (0, 1, 3):
            whole = rs.resample(src, A, shape, order=order, cval=CVAL, layout=layout)
            assert np.array_equal(whole, rs.resample(src, A, shape, order=order, cval=CVAL, layout=layout))           # run to run
            for work in (lo, 2 * lo, 4 * lo + 100):                                                                    # 1, 2 and 4 series per chunk
                assert np.array_equal(whole, rs.resample(src, A, shape, order=order, cval=CVAL, layout=layout, max_work_bytes=work)), (layout, order, work)
            single = np.stack([rs.resample(v[s], A, shape, order=order, cval=CVAL) for s in range(S)])                 # one by one
            assert np.array_equal(from_layout(whole, layout), single), (layout, order)
    # tensors in, tensors out, on the same device
    t = torch.as_tensor(v, device="cuda")
    out, ins = rs.resample(t, A, shape, order=3, cval=CVAL, return_inside=True)
    assert out.is_cuda and ins.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), rs.resample(v, A, shape, order=3, cval=CVAL))


def test_offsets_beyond_2_31_elements(rs):
    """17 series on a 512^3 destination: 2.28e9 elements, so the element offsets of the last series (series-major) and of the last voxels
    (voxel-major) do not fit 32 bits; compared on the device with the same series resampled alone"""
    dims, shape, S = (9, 8, 7), (512, 512, 512), 17
    v = rn.volume(np.random.default_rng(17), dims, S)
    A = rn.rotated(dims, shape)
    alone = {s: rs.resample(torch.as_tensor(v[s], device="cuda"), A, shape, order=1, cval=CVAL) for s in (0, S - 1)}
    assert bool((alone[0] != CVAL).any()) and bool((alone[0] == CVAL).any())
    for layout in ("series", "voxel"):
        out = rs.resample(torch.as_tensor(to_layout(v, layout), device="cuda"), A, shape, order=1, cval=CVAL, layout=layout)
        assert out.numel() == S * 2 ** 27 > 2 ** 31
        for s, one in alone.items():
            assert torch.equal(out[s] if layout == "series" else out[..., s], one), (layout, s)
        del out


def test_optional_outputs_and_refusals_leave_the_outputs_alone(rs):
    _lib = importlib.import_module(PKG + "._lib")
    L = _lib.lib()
    dims, shape, S = (5, 4, 6), (4, 5, 3), 2
    rng = np.random.default_rng(9)
    v = rn.volume(rng, dims, S)
    A = np.ascontiguousarray(rn.transforms(dims, shape)["rotated"])
    Ap = A.ctypes.data_as(_lib._dp)
    i3 = lambda d: (C.c_int32 * 3)(*d)
    src = torch.as_tensor(v, device="cuda")
    n_src, n_dst = int(np.prod(dims)), int(np.prod(shape))
    sentinel = 12345.0
    dst = torch.full((S,) + shape, sentinel, dtype=torch.float64, device="cuda")
    ins = torch.full(shape, 77, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(order=1, sd=dims, n=S, sp=None, svs=1, sss=n_src, dd=shape, a=Ap, dp=None, dvs=1, dss=n_dst, inside=None, work=0):
        return L.met2_resample(0, order, i3(sd), n, src.data_ptr() if sp is None else sp, svs, sss, i3(dd), a, CVAL, dst.data_ptr() if dp is None else dp,
                               dvs, dss, inside, work, stream)

    nanA = np.ascontiguousarray(np.full((3, 4), np.nan)).ctypes.data_as(_lib._dp)
    refused = [call(order=2, inside=ins.data_ptr()), call(sd=(5, 4, 513), inside=ins.data_ptr()), call(dd=(4, 0, 3), inside=ins.data_ptr()),
               call(n=0, inside=ins.data_ptr()), call(n=32769, inside=ins.data_ptr()), call(a=nanA, inside=ins.data_ptr()),
               call(svs=0, inside=ins.data_ptr()), call(dss=n_dst - 1, inside=ins.data_ptr()), call(dp=src.data_ptr(), inside=ins.data_ptr()),
               call(order=3, work=-1, inside=ins.data_ptr()), call(order=3, work=8 * n_src - 8, inside=ins.data_ptr())]
    torch.cuda.synchronize()
    assert all(rc in (-1, -2) for rc in refused) and refused[1] == -2 and refused[4] == -2
    assert bool((dst == sentinel).all()) and bool((ins == 77).all())
    lab = torch.zeros(dims, dtype=torch.int32, device="cuda")
    lout = torch.full(shape, 4242, dtype=torch.int32, device="cuda")
    assert L.met2_resample_labels(0, i3((5, 4, 600)), lab.data_ptr(), i3(shape), Ap, 0, lout.data_ptr(), ins.data_ptr(), stream) == -2
    assert L.met2_resample_labels(0, i3(dims), lab.data_ptr(), i3(shape), nanA, 0, lout.data_ptr(), ins.data_ptr(), stream) == -1
    coef = torch.full((S,) + dims, sentinel, dtype=torch.float64, device="cuda")
    assert L.met2_resample_prefilter(0, i3(dims), 0, src.data_ptr(), 1, n_src, coef.data_ptr(), stream) == -1
    assert L.met2_resample_prefilter(0, i3(dims), S, src.data_ptr(), 1, 0, coef.data_ptr(), stream) == -1
    torch.cuda.synchronize()
    assert bool((lout == 4242).all()) and bool((ins == 77).all()) and bool((coef == sentinel).all())
    # the optional outputs may be NULL: inside of all three orders and of the labels
    for order in (0, 1, 3):
        assert call(order=order) == 0
        torch.cuda.synchronize()
        with_ins = rs.resample(v, A, shape, order=order, cval=CVAL, return_inside=True)[0]
        assert np.array_equal(dst.cpu().numpy(), with_ins) and bool((ins == 77).all())
    assert L.met2_resample_labels(0, i3(dims), lab.data_ptr(), i3(shape), Ap, 5, lout.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(lout.cpu().numpy(), np.where(rn.inside_map(A, dims, shape) > 0, 0, 5))
    assert L.met2_resample_work_bytes(3, i3(dims), S, None, None) == 0


def test_the_filters(rs, motor):
    dims, shape = (9, 8, 7), rn.dst_dims((9, 8, 7))
    v, refs = reference(dims)
    A = rn.transforms(dims, shape)["rotated"]
    echo = to_layout(v, "voxel")
    got, ins = motor.resample_filter(echo, A, shape, order=3, cval=CVAL, return_inside=True)
    assert got.shape == shape + (9,) and np.array_equal(got, rs.resample(echo, A, shape, order=3, cval=CVAL, layout="voxel"))
    assert np.array_equal(ins, refs["rotated", 3][1])
    assert np.array_equal(motor.resample_filter(v, A, shape, series_axis=0), rs.resample(v, A, shape, order=1))
    assert np.array_equal(motor.resample_filter(v[0], A, shape, order=0), rs.resample(v[0], A, shape, order=0))
    t = motor.resample_filter(torch.as_tensor(echo, device="cuda"), A, shape, order=1, cval=CVAL, max_work_bytes=0)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), rs.resample(echo, A, shape, order=1, cval=CVAL, layout="voxel"))
    lab = np.random.default_rng(2).integers(0, 50, dims)
    assert np.array_equal(motor.resample_labels_filter(lab, A, shape, fill=3), rn.resample_labels(lab, A, shape, fill=3))


def test_atlas_stats_filter(rs, motor):
    """a label image on a grid of its own, rotated and finer than the maps': every field equals label_stats_filter on the restatement's labels"""
    rng = np.random.default_rng(21)
    shape, n_t2 = (7, 6, 5), 5
    res = {k: rng.random(shape) for k in motor.STAT_QUANTITIES}
    res["MWF"][2, 3, 1] = np.nan
    res["fsol_4D"] = rng.random(shape + (n_t2,))
    res["T2s"] = np.logspace(1, 3, n_t2)
    c, s = np.cos(np.deg2rad(8.0)), np.sin(np.deg2rad(8.0))
    affine = np.array([[2.0, 0, 0, -7.0], [0, 2.0, 0, -6.0], [0, 0, 3.0, -7.5], [0, 0, 0, 1.0]])
    labels_affine = np.array([[c, -s, 0, -8.0], [s, c, 0, -7.0], [0, 0, 1.0, -8.0], [0, 0, 0, 1.0]]) @ np.diag([0.9, 1.1, 1.2, 1.0])
    ldims = (17, 13, 14)
    labels = (rng.integers(0, 4, (6, 5, 5)).repeat(3, 0).repeat(3, 1).repeat(3, 2)[:17, :13, :14] * 5).astype(np.int16)
    world = np.eye(4)
    world[:3, 3] = (0.5, -0.25, 1.0)
    A = rs.voxel_matrix(affine, labels_affine, world)
    want_lab = rn.resample_labels(labels, A, shape, fill=0)
    assert labels.shape == ldims and 0 < (want_lab > 0).sum() and (rn.inside_map(A, ldims, shape) == 0).any()     # some of the maps lie outside the atlas
    got = motor.atlas_stats_filter(res, labels, labels_affine, affine, world=world, q=(0.1, 0.5, 0.9))
    want = motor.label_stats_filter(res, want_lab, q=(0.1, 0.5, 0.9))
    assert np.array_equal(got["labels_resampled"], want_lab) and got["labels_resampled"].dtype == np.int32
    assert set(got) == set(want) | {"labels_resampled"}
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True) if k != "quantities" else got[k] == want[k], k
