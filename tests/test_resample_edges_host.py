"""Host-side checks of the cases tests/test_gpu_resample_edges.py runs on the device (no GPU): what each series count and each long axis is
there for, stated from the launch arithmetic of met2_resample.hip; every resampling case has at least MIN_INSIDE inside voxels and one
outside ("scale" on a long axis may keep every voxel inside; "half" beside it never does); and the fp64 leg of the restatement (tests/tools/resample_numpy.py) lies within 1e-13 max|src| of its long-double leg on those
inputs, so the device's bound of 1e-12 max|src| leaves the reference a tenth of itself at the most."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import resample_numpy as rn                                        # noqa: E402

RESTATEMENT_BOUND = 1e-13


def test_what_each_series_count_and_axis_is_there_for():
    S = rn.EDGE_N_SERIES
    assert S == (4, 5, 31, 32, 33, 48, 60, 64, 65, 120)
    assert [rn.group_width(s) for s in S] == [4, 8, 32, 32, 64, 64, 64, 64, 64, 64]
    assert [rn.group_turns(s) for s in S] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 2]            # 65 and 120: a second turn of the series loop
    assert [rn.series_tiles(s) for s in S] == [(1, 4), (1, 5), (1, 31), (1, 32), (2, 1), (2, 16), (2, 28), (2, 32), (3, 1), (4, 24)]
    assert [rn.group_width(s) for s in rn.N_SERIES if s >= 4] == [8, 16]                # what tests/test_gpu_resample.py holds against the reference
    for c, tail in zip(rn.CHUNK_SERIES, (21, 40)):
        assert 120 - (-(-120 // c) - 1) * c == tail
    assert (rn.series_tiles(33), rn.series_tiles(21), rn.series_tiles(40)) == ((2, 1), (1, 21), (2, 8))
    assert [int(np.prod(d)) for d in rn.GATHER_DIMS] == [24, 64, 65, 504] and rn.GATHER_DIMS[2][2] == 1
    want = {"nz512": (15, 2, 1), "nz125": (64, 2, 1), "nz126": (63, 2, 2)}
    for name, dims, series in rn.LONG_AXES:
        assert max(dims) <= 512 and max(series) * int(np.prod(dims)) <= 4 * 2048
        if name in want:
            assert rn.z_tiles(dims[2], max(series) * dims[0] * dims[1]) == want[name], name
    assert rn.z_tiles(512, 4)[0] * 513 * 8 == 61560
    assert rn.z_tiles(65, 12) == (64, 1, 12) and rn.z_tiles(129, 12)[0] == 62           # the tiles of the existing module


def floors(ins, where, outside=True):
    assert int(ins.sum()) >= rn.MIN_INSIDE and int((ins == 0).sum()) >= int(outside), (where, int(ins.sum()), ins.size)


@pytest.mark.parametrize("dims", rn.EDGE_DIMS)
def test_the_series_count_cases(dims):
    S = max(rn.EDGE_N_SERIES)
    v = rn.edge_volume(dims, S)
    vmax = np.abs(v[:min(rn.EDGE_N_SERIES)]).max()                                      # the smallest max|src| of any slice the GPU test takes
    shape = rn.dst_dims(dims)
    T = rn.transforms(dims, shape)
    for name in rn.EDGE_TRANSFORMS:
        floors(rn.inside_map(T[name], dims, shape), (dims, name))
        for order in (0, 1, 3):
            a = rn.resample(v, T[name], shape, order, cval=-7.5)
            b = rn.resample(v, T[name], shape, order, cval=-7.5, dtype=np.longdouble)
            if order == 0:
                assert np.array_equal(a, b)
            else:
                err = np.abs(a - b).max()
                print("%s order %d: fp64 to long double %.2e" % ((dims, name), order, err / vmax))
                assert err <= RESTATEMENT_BOUND * vmax, (dims, name, order)


@pytest.mark.parametrize("dims", rn.GATHER_DIMS)
def test_the_prefilter_cases(dims):
    v = rn.edge_volume(dims, max(rn.EDGE_N_SERIES))
    vmax = np.abs(v[:min(rn.EDGE_N_SERIES)]).max()
    assert np.abs(rn.prefilter(v) - rn.prefilter(v, np.longdouble)).max() <= RESTATEMENT_BOUND * vmax


def test_the_stride_and_chunk_cases_are_series_count_cases():
    assert (9, 8, 7) in rn.EDGE_DIMS and "rotated" in rn.EDGE_TRANSFORMS and set(rn.STRIDE_N_SERIES) <= set(rn.EDGE_N_SERIES)


@pytest.mark.parametrize("name,dims,series", rn.LONG_AXES, ids=[c[0] for c in rn.LONG_AXES])
def test_the_long_axis_cases(name, dims, series):
    v = rn.edge_volume(dims, max(series))
    vmax = np.abs(v[:1]).max()
    err = np.abs(rn.prefilter(v) - rn.prefilter(v, np.longdouble)).max()
    print("%s prefilter: fp64 to long double %.2e" % (name, err / vmax))
    assert err <= RESTATEMENT_BOUND * vmax
    shape = rn.dst_dims(dims)
    T = rn.transforms(dims, shape)
    for t in rn.LONG_TRANSFORMS:
        floors(rn.inside_map(T[t], dims, shape), (name, t), outside=t == "half")         # "scale" keeps all of nz125 and nz126 inside
        err = np.abs(rn.resample(v, T[t], shape, 3, cval=-7.5) - rn.resample(v, T[t], shape, 3, cval=-7.5, dtype=np.longdouble)).max()
        print("%s %s order 3: fp64 to long double %.2e" % (name, t, err / vmax))
        assert err <= RESTATEMENT_BOUND * vmax, (name, t)
