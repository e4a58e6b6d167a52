"""The affine resampling on the device at the sizes tests/test_gpu_resample.py leaves out, against the long-double restatement
(tests/tools/resample_numpy.py; tests/test_resample_edges_host.py bounds its fp64 leg at 1e-13 max|src| on these inputs and asserts what
each case is there for): the inside map, order 0 and the labels equal in every voxel, orders 1 and 3 and the prefilter within 1e-12 max|src|.
  series counts   4 .. 120 series (echo data: 32 and 48, spectra: 60 and 120) in both layouts at all three orders: rs_group_kernel at widths
                  4, 8, 32 and 64 and in a second turn of its series loop (65, 120); rs_gather_kernel<true> over 1 .. 4 series tiles with
                  full and partial last tiles; voxel-major, series-major and every series alone give the same bits
  prefilter       the gather's voxel tiles: one partial (24 voxels), one full (64), 65 voxels with nz = 1, 504
  chunks          order 3 of 120 series in chunks of 33 and 40: a chunk wider than a series tile, a tail of 21
  strides         the C entries on padded and mixed layouts: the same bits as the contiguous call, the destination's padding untouched
  long axes       lines of 512 samples along x, y and z (the z pass's tile of 15 lines and a tile of one), and the z tile's step from
                  64 to 63 lines between nz = 125 and 126
  labels          INT32_MIN and INT32_MAX pass through unchanged
Measured on an MI355X (profiles/resample_edges_parity.json), relative to max|src|: series counts order 1 1.9e-16, order 3 1.2e-15; prefilter
at the gather's tiles 1.1e-14; long axes order 3 1.3e-15, prefilter 1.2e-14 (the fp64 restatement itself: 1.3e-14 at nz = 512).  No case
misses a check: none of these paths turned out to be wrong.
With MET2_RESAMPLE_EDGES_PARITY_OUT=<file> the module writes its measured maxima per section there as JSON."""
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
SENTINEL = 12345.0
S_MAX = max(rn.EDGE_N_SERIES)
MAXIMA = {"series_counts": {"order1": 0.0, "order3": 0.0}, "prefilter_tiles": {"prefilter": 0.0},
          "long_axes": {"order3": 0.0, "prefilter": 0.0}}


@pytest.fixture(scope="module")
def rs():
    yield importlib.import_module(PKG + ".resample")
    path = os.environ.get("MET2_RESAMPLE_EDGES_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"bound": BOUND, "relative_to": "max|src| of the case", "max_abs_error_over_max_src": MAXIMA}, f, indent=1)


def note(section, key, err, vmax):
    MAXIMA[section][key] = max(MAXIMA[section][key], float(err / vmax))


def to_layout(v, layout):
    return np.array(v if layout == "series" else np.moveaxis(v, 0, -1), order="C")


def from_layout(a, layout):
    return a if layout == "series" else np.moveaxis(a, -1, 0)


def dim_id(dims):
    return "x".join(str(n) for n in dims)


_SRC, _REF, _PRE, _ALONE = {}, {}, {}, {}


def source(dims, n_series=S_MAX):
    if (dims, n_series) not in _SRC:
        v = rn.edge_volume(dims, n_series)
        v.setflags(write=False)
        _SRC[dims, n_series] = v
    return _SRC[dims, n_series]


def reference(dims, name, order, n_series=S_MAX):
    """(ref long double [n_series, ...], inside) of one source grid, transform and order, computed once and sliced per series count"""
    key = (dims, name, order, n_series)
    if key not in _REF:
        shape = rn.dst_dims(dims)
        A = rn.transforms(dims, shape)[name]
        _REF[key] = rn.resample(source(dims, n_series), A, shape, order, cval=CVAL, dtype=np.longdouble, return_inside=True)
    return _REF[key]


def prefilter_reference(dims, n_series=S_MAX):
    if (dims, n_series) not in _PRE:
        _PRE[dims, n_series] = rn.prefilter(source(dims, n_series), np.longdouble)
    return _PRE[dims, n_series]


def alone(rs, dims, name, order):
    """every series of the source resampled in a call of its own, on the device, once: [S_MAX, ...]"""
    key = (dims, name, order)
    if key not in _ALONE:
        shape = rn.dst_dims(dims)
        A = rn.transforms(dims, shape)[name]
        t = torch.as_tensor(source(dims).copy(), device="cuda")
        _ALONE[key] = torch.stack([rs.resample(t[s], A, shape, order=order, cval=CVAL) for s in range(S_MAX)]).cpu().numpy()
    return _ALONE[key]


def check_floors(ins, where, outside=True):
    assert int(ins.sum()) >= rn.MIN_INSIDE and int((ins == 0).sum()) >= int(outside), where


def test_what_each_series_count_is_there_for():
    S = rn.EDGE_N_SERIES
    assert {s: rn.group_width(s) for s in S} == {4: 4, 5: 8, 31: 32, 32: 32, 33: 64, 48: 64, 60: 64, 64: 64, 65: 64, 120: 64}
    assert {s: rn.group_turns(s) for s in S if rn.group_turns(s) > 1} == {65: 2, 120: 2}
    assert {s: rn.series_tiles(s) for s in S} == {4: (1, 4), 5: (1, 5), 31: (1, 31), 32: (1, 32), 33: (2, 1), 48: (2, 16), 60: (2, 28),
                                                  64: (2, 32), 65: (3, 1), 120: (4, 24)}


# ---------------------------------------------------------------- 1. series counts, both layouts, all three orders

@pytest.mark.parametrize("order", (0, 1, 3), ids=lambda o: "order%d" % o)
@pytest.mark.parametrize("layout", ("voxel", "series"))
@pytest.mark.parametrize("S", rn.EDGE_N_SERIES, ids=lambda s: "S%d" % s)
@pytest.mark.parametrize("name", rn.EDGE_TRANSFORMS)
@pytest.mark.parametrize("dims", rn.EDGE_DIMS, ids=dim_id)
def test_series_counts(rs, dims, name, S, layout, order):
    v = source(dims)[:S].copy()
    vmax = np.abs(v).max()
    shape = rn.dst_dims(dims)
    A = rn.transforms(dims, shape)[name]
    ref, ref_ins = reference(dims, name, order)
    check_floors(ref_ins, (dims, name))
    got, ins = rs.resample(to_layout(v, layout), A, shape, order=order, cval=CVAL, layout=layout, return_inside=True)
    assert got.shape == ((S,) + shape if layout == "series" else shape + (S,))
    got = from_layout(got, layout)
    assert np.array_equal(ins, ref_ins)
    if order == 0:
        assert np.array_equal(got, ref[:S])
    else:
        err = np.abs(got - ref[:S]).max()
        note("series_counts", "order%d" % order, err, vmax)
        print("max error %.3e of max|src|" % (err / vmax))
        assert err <= BOUND * vmax
    # the same bits as every series in a call of its own: so in both layouts, through either interpolation kernel and any group width
    assert np.array_equal(got, alone(rs, dims, name, order)[:S])


# ---------------------------------------------------------------- 2. the prefilter stage at the gather's tile edges

@pytest.mark.parametrize("S", rn.EDGE_N_SERIES, ids=lambda s: "S%d" % s)
@pytest.mark.parametrize("dims", rn.GATHER_DIMS, ids=lambda d: "gather-%dvox-%s" % (int(np.prod(d)), dim_id(d)))
def test_prefilter_at_the_gathers_tile_edges(rs, dims, S):
    v = source(dims)[:S].copy()
    vmax = np.abs(v).max()
    ref = prefilter_reference(dims)[:S]
    got = {}
    for layout in ("voxel", "series"):
        got[layout] = rs.prefilter(to_layout(v, layout), layout=layout)
        err = np.abs(got[layout] - ref).max()
        note("prefilter_tiles", "prefilter", err, vmax)
        print("%s max error %.3e of max|src|" % (layout, err / vmax))
        assert got[layout].shape == (S,) + dims and err <= BOUND * vmax, layout
    assert np.array_equal(got["voxel"], got["series"])


# ---------------------------------------------------------------- 3. order-3 chunks across series tiles

@pytest.mark.parametrize("layout", ("voxel", "series"))
@pytest.mark.parametrize("chunk", rn.CHUNK_SERIES, ids=lambda c: "chunk%d" % c)
def test_order3_chunks_across_series_tiles(rs, chunk, layout):
    dims = (9, 8, 7)
    shape = rn.dst_dims(dims)
    A = rn.transforms(dims, shape)["rotated"]
    src = to_layout(source(dims), layout)
    lo, dflt = rs.work_bytes(3, dims, S_MAX)
    assert dflt == S_MAX * lo and (chunk * lo + 100) // lo == chunk
    whole, ins = rs.resample(src, A, shape, order=3, cval=CVAL, layout=layout, return_inside=True)
    got, got_ins = rs.resample(src, A, shape, order=3, cval=CVAL, layout=layout, return_inside=True, max_work_bytes=chunk * lo + 100)
    assert np.array_equal(got, whole)
    assert np.array_equal(got_ins, ins) and np.array_equal(ins, reference(dims, "rotated", 3)[1])      # written by the first chunk only
    assert np.array_equal(from_layout(whole, layout), alone(rs, dims, "rotated", 3))


# ---------------------------------------------------------------- 4. general strides through the C entries

def strided(v, vs, ss, fill, tail=16):
    """v [S, n] at element v_index vs + s ss of a flat buffer, `fill` everywhere else -> (buffer, the elements' offsets [S, n])"""
    S, n = v.shape
    off = np.arange(S)[:, None] * ss + np.arange(n)[None, :] * vs
    assert np.unique(off).size == off.size
    buf = np.full(int(off.max()) + 1 + tail, fill, dtype=np.float64)
    buf[off] = v
    return buf, off


def stride_cases(S, n_src, n_dst):
    """name -> ((svs, sss), (dvs, dss))"""
    vox_s, ser_s, vox_d, ser_d = (S, 1), (1, n_src), (S, 1), (1, n_dst)
    return {"pad-src-voxel": ((S + 3, 1), vox_d), "pad-src-series": ((1, n_src + 5), ser_d), "pad-src-both": ((2, 2 * n_src + 1), ser_d),
            "pad-dst-voxel": (vox_s, (S + 2, 1)), "pad-dst-series": (ser_s, (1, n_dst + 7)),
            "mixed-voxel-to-series": (vox_s, ser_d), "mixed-series-to-voxel": (ser_s, vox_d)}


STRIDE_CASES = tuple(stride_cases(1, 1, 1))


@pytest.mark.parametrize("order", (0, 1, 3), ids=lambda o: "order%d" % o)
@pytest.mark.parametrize("S", rn.STRIDE_N_SERIES, ids=lambda s: "S%d" % s)
@pytest.mark.parametrize("case", STRIDE_CASES)
def test_strides_through_the_c_entry(rs, case, S, order):
    _lib = importlib.import_module(PKG + "._lib")
    dims = (9, 8, 7)
    shape = rn.dst_dims(dims)
    n_src, n_dst = int(np.prod(dims)), int(np.prod(shape))
    A = np.ascontiguousarray(rn.transforms(dims, shape)["rotated"])
    v = source(dims)[:S].copy()
    want, want_ins = rs.resample(v, A, shape, order=order, cval=CVAL, return_inside=True)
    (svs, sss), (dvs, dss) = stride_cases(S, n_src, n_dst)[case]
    rs.check_strides(S, n_src, svs, sss)
    rs.check_strides(S, n_dst, dvs, dss, destination=True)
    sbuf, _ = strided(v.reshape(S, n_src), svs, sss, np.nan)
    dbuf, doff = strided(np.full((S, n_dst), SENTINEL), dvs, dss, SENTINEL)
    src, dst = torch.as_tensor(sbuf, device="cuda"), torch.as_tensor(dbuf, device="cuda")
    ins = torch.full((n_dst + 16,), 77, dtype=torch.uint8, device="cuda")
    i3 = lambda d: (C.c_int32 * 3)(*d)
    _lib.check(_lib.lib().met2_resample(0, order, i3(dims), S, src.data_ptr(), svs, sss, i3(shape), A.ctypes.data_as(_lib._dp), CVAL, dst.data_ptr(),
                                        dvs, dss, ins.data_ptr(), 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out, ins = dst.cpu().numpy(), ins.cpu().numpy()
    assert np.array_equal(out[doff].reshape((S,) + shape), want)
    padding = np.ones(out.size, dtype=bool)
    padding[doff] = False
    assert padding.sum() == out.size - S * n_dst and (padding.sum() > 16) == case.startswith("pad-dst")
    assert np.all(out[padding] == SENTINEL)
    assert np.array_equal(ins[:n_dst].reshape(shape), want_ins) and np.all(ins[n_dst:] == 77)
    assert np.array_equal(sbuf, src.cpu().numpy(), equal_nan=True)                                     # the source is only read


@pytest.mark.parametrize("S", rn.STRIDE_N_SERIES, ids=lambda s: "S%d" % s)
@pytest.mark.parametrize("case", [c for c in STRIDE_CASES if c.startswith("pad-src")])
def test_prefilter_strides_through_the_c_entry(rs, case, S):
    _lib = importlib.import_module(PKG + "._lib")
    dims = (9, 8, 7)
    n_src = int(np.prod(dims))
    v = source(dims)[:S].copy()
    want = rs.prefilter(v)
    (svs, sss), _ = stride_cases(S, n_src, 1)[case]
    sbuf, _ = strided(v.reshape(S, n_src), svs, sss, np.nan)
    src = torch.as_tensor(sbuf, device="cuda")
    coef = torch.full((S * n_src + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().met2_resample_prefilter(0, (C.c_int32 * 3)(*dims), S, src.data_ptr(), svs, sss, coef.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = coef.cpu().numpy()
    assert np.array_equal(out[:S * n_src].reshape((S,) + dims), want) and np.all(out[S * n_src:] == SENTINEL)


# ---------------------------------------------------------------- 5. long axes

LONG_CASES = [pytest.param(dims, max(series), S, id="%s-S%d" % (name, S)) for name, dims, series in rn.LONG_AXES for S in series]


@pytest.mark.parametrize("dims,n_series,S", LONG_CASES)
def test_long_axes_prefilter(rs, dims, n_series, S):
    v = source(dims, n_series)[:S].copy()
    vmax = np.abs(v).max()
    ref = prefilter_reference(dims, n_series)[:S]
    got = {}
    for layout in ("voxel", "series"):
        got[layout] = rs.prefilter(to_layout(v, layout), layout=layout)
        err = np.abs(got[layout] - ref).max()
        note("long_axes", "prefilter", err, vmax)
        print("%s max error %.3e of max|src|" % (layout, err / vmax))
        assert got[layout].shape == (S,) + dims and err <= BOUND * vmax, layout
    assert np.array_equal(got["voxel"], got["series"])
    assert np.array_equal(rs.prefilter(v[S - 1]), got["series"][S - 1])


@pytest.mark.parametrize("name", rn.LONG_TRANSFORMS)
@pytest.mark.parametrize("dims,n_series,S", LONG_CASES)
def test_long_axes_order3(rs, dims, n_series, S, name):
    v = source(dims, n_series)[:S].copy()
    vmax = np.abs(v).max()
    shape = rn.dst_dims(dims)
    A = rn.transforms(dims, shape)[name]
    ref, ref_ins = reference(dims, name, 3, n_series)
    check_floors(ref_ins, (dims, name), outside=name == "half")         # "scale" keeps every voxel of nz125 and nz126 inside
    got = {}
    for layout in ("voxel", "series"):
        out, ins = rs.resample(to_layout(v, layout), A, shape, order=3, cval=CVAL, layout=layout, return_inside=True)
        got[layout] = from_layout(out, layout)
        assert np.array_equal(ins, ref_ins), layout
        err = np.abs(got[layout] - ref[:S]).max()
        note("long_axes", "order3", err, vmax)
        print("%s max error %.3e of max|src|" % (layout, err / vmax))
        assert err <= BOUND * vmax, layout
    assert np.array_equal(got["voxel"], got["series"])


# ---------------------------------------------------------------- 6. labels at the ends of int32

def test_labels_at_the_ends_of_int32(rs):
    dims = (9, 8, 7)
    shape = rn.dst_dims(dims)
    A = rn.transforms(dims, shape)["rotated"]
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    lab = np.random.default_rng(6).choice(np.array([lo, lo + 1, -1, 0, 1, hi - 1, hi], dtype=np.int32), size=dims)
    for fill in (lo, hi, 0):
        got, ins = rs.resample_labels(lab, A, shape, fill=fill, return_inside=True)
        want = rn.resample_labels(lab, A, shape, fill=fill)
        assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(ins, rn.inside_map(A, dims, shape))
        inside = got[ins.astype(bool)]
        assert (inside == lo).sum() > 10 and (inside == hi).sum() > 10 and np.all(got[ins == 0] == fill)
    dev = rs.resample_labels(torch.as_tensor(lab, device="cuda"), A, shape, fill=lo)
    assert dev.dtype == torch.int32 and np.array_equal(dev.cpu().numpy(), rn.resample_labels(lab, A, shape, fill=lo))
