"""The two whole-volume filters of met2_prefilter.hip, met2_nesma (nesma_kernel) and met2_smooth_separable (smooth_axis_kernel), where
their kernels branch.  Both are bit-identical to their reference, so every comparison here is np.array_equal: no tolerance anywhere.

NESMA (reference: oracle.nesma, the C restatement of motor:305-333, which test_nesma_filter_and_driver_golden holds against rows of the
reference's driver and the CPU part here against the same lines written with numpy):
  A  every launch of met2_nesma's dispatch on the echo count (tools/nesma_cases.DISPATCH restates it), every branch of the row sum
     (fewer than 8 echoes, 8 running sums, with and without the in-order tail) and every z-run length 1..12, on two-class volumes with
     2.2 % noise: 10-19 % of the window pairs of the 6x7x13 volume then lie within 10 % of the 2.5 % threshold (asserted on the CPU), so
     a distance sum that loses one echo changes decisions.
  B  integer volumes on which RE is exactly 2.5 for > 5000 pairs per case (every step exact in int64 and in fp64, so the decision and
     the mean are known without any floating-point sum), negative sums, zero sums of non-zero echoes, NaN and +-inf echoes.
     One echo: numpy's np.mean over the similar rows is then a contiguous reduction, summed pairwise and not in window order; the oracle
     and the kernel once added in window order (1 ulp off), found by the comparison with numpy here, and nt = 1 has a launch of its own.
Gaussian smoothing (reference: scipy.ndimage.gaussian_filter):
  C  a volume of more than 256 * 64 * 256 elements, where the kernel's grid-stride loop takes a second trip; the entry without a work
     array (own allocation, stream wait, free); the entry's refusals, which must leave the output untouched.

The CPU tests assert the conditions on the inputs: which launch each echo count selects, the share of pairs near the threshold, the number
of exact ties, the z-runs that occur, the element count above one grid.  They print what they measure (pytest -s).
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import nesma_cases as nc  # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"
# the shared inputs are read-only numpy arrays; the package copies them to the device and never writes to them
pytestmark = pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")
ONE_GRID = 256 * 64 * 256                       # smooth_axis_kernel's launch cap: workgroups x threads
SHAPE_PAST_ONE_GRID = (65, 40, 41, 41)
SHAPE_NO_WORK = (33, 7, 20, 3)
_ID_A = ["%dx%dx%d-nt%d" % (s + (nt,)) for s, nt in nc.CASES_A]
_WANT = {}


def want_a(oracle, shape, nt):
    """oracle.nesma of case A, computed once and shared (read-only)"""
    if (shape, nt) not in _WANT:
        d, m, _, _ = nc.case_a(shape, nt)
        w = oracle.nesma(d, m.astype(float), nthreads=8)
        w.setflags(write=False)
        _WANT[shape, nt] = w
    return _WANT[shape, nt]


# ------------------------------------------------------------------ CPU: the conditions on the inputs
def test_every_launch_and_sum_branch_is_visited():
    # the dispatch of met2_nesma, restated: nt == 1, nt == 32, nt < 32, nt == 48, nt <= 64, nt <= 128, first match wins
    assert [nc.launch(nt) for nt in (1, 2, 31, 32, 33, 47, 48, 49, 64, 65, 128)] == \
        ["one echo", "<1,2,0>", "<1,2,0>", "<1,2,32>", "<1,1,0>", "<1,1,0>", "<1,1,48>", "<1,1,0>", "<1,1,0>", "<2,1,0>", "<2,1,0>"]
    hit = {name: set() for name, _ in nc.DISPATCH}
    for shape, nt in nc.CASES_A:
        hit[nc.launch(nt)].add((shape, nt))
    for nt in nc.NT_TIES:
        hit[nc.launch(nt)].add((nc.SHAPE_TIES, nt))
    hit["one echo"].add((nc.ONE_ECHO_SHAPE, 1))
    for name, cases in hit.items():
        counts = {nt for _, nt in cases}
        # the launches for one echo count (1, 32, 48) can only see that count: two inputs each or more; the others two counts or more
        assert len(cases) >= 2 and (name in ("one echo", "<1,2,32>", "<1,1,48>") or len(counts) >= 2), (name, cases)
        print("MEASURED nesma launch %s: %d inputs, echo counts %s" % (name, len(cases), sorted(counts)))
    assert hit["<1,2,0>"] >= {(nc.BIG, nt) for nt in (7, 8, 9, 16, 31)}
    assert hit["<1,1,0>"] >= {(nc.BIG, nt) for nt in (33, 40, 63, 64)}
    assert hit["<2,1,0>"] >= {(nc.BIG, nt) for nt in (65, 72, 127, 128)}
    # the two-neighbours-per-load kernel with a run-time count: all three paths of its row sum, and runs past 8 (S1, live1)
    assert {nc.sum_branch(nt) for _, nt in hit["<1,2,0>"]} >= {"in order", "8 sums", "8 sums + tail of 1", "8 sums + tail of 7"}
    for name in hit:
        assert any(max(nc.z_runs(shape)) > 8 for shape, _ in hit[name]) and any(max(nc.z_runs(shape)) <= 8 for shape, _ in hit[name])
    # every run length 1..12 occurs, and x and y windows clipped on both sides, on one side, and not at all
    assert nc.z_runs(nc.BIG) == [6, 7, 8, 9, 10, 11, 12]
    assert [nc.z_runs((3, 4, nz)) for nz in (1, 2, 3, 5, 9)] == [[1], [2], [3], [5], [6, 7, 8, 9]]
    assert 6 * 7 * 13 % 4 != 0 and 6 * 7 * 13 % 32 != 0


@pytest.mark.parametrize("shape,nt", nc.CASES_A, ids=_ID_A)
def test_case_a_lies_near_the_threshold(oracle, shape, nt):
    d, m, three, zero = nc.case_a(shape, nt)
    near, similar, pairs = nc.shares(d, m)
    print("MEASURED nesma A %s nt=%d launch %s, row sum %s, z-runs %s: %d pairs, %.3f within 10 %% of 2.5, %.3f similar, %.2f masked out"
          % (shape, nt, nc.launch(nt), nc.sum_branch(nt), nc.z_runs(shape), pairs, near, similar, np.mean(m == 0)))
    assert m[three] == 3 and m[zero] == 1 and not d[zero].any() and d[three].all()
    if shape == nc.BIG:
        assert 0.1 < np.mean(m == 0) < 0.3
        if nt >= 8:
            assert near >= 0.10 and 0.10 <= similar <= 0.60
    want = want_a(oracle, shape, nt)
    assert np.all(np.isnan(want[zero])) and not want[m != 1].any()
    assert np.isfinite(want[(m == 1) & d.any(axis=-1)]).all()
    assert np.array_equal(want, nc.nesma_numpy(d, m), equal_nan=True)                    # the oracle against the reference's lines in numpy


@pytest.mark.parametrize("nt", nc.NT_TIES)
def test_tie_volumes_hold_exact_ties(oracle, nt):
    base, u = nc.tie_vectors(nt)
    assert base.sum() == 8000 and u.sum() == 0 and np.abs(u).sum() == 50 and np.count_nonzero(u) == min(nt, 50) and u[0] != 0 and u[-1] != 0
    if nt == 2:
        assert u.tolist() == [25, -25]
    d = nc.tie_case(nt)
    assert d.dtype == np.int64 and d.shape == nc.SHAPE_TIES + (nt,) and np.all(d.sum(axis=-1) == 8000)
    ref, ties, pairs = nc.tie_reference(nt)
    print("MEASURED nesma ties nt=%d launch %s, row sum %s: %d of %d pairs have RE == 2.5 exactly" % (nt, nc.launch(nt), nc.sum_branch(nt), ties, pairs))
    assert pairs == 48000 and ties >= 1000
    # exact in fp64 as well: the oracle and numpy's floating point agree with the integer arithmetic bit for bit
    ones = np.ones(nc.SHAPE_TIES)
    assert np.array_equal(oracle.nesma(d.astype(np.float64), ones), ref)
    assert np.array_equal(nc.nesma_numpy(d.astype(np.float64), ones), ref)


def test_one_echo_input_on_the_cpu(oracle):
    # at one echo np.mean over the similar rows is a contiguous reduction, which numpy sums pairwise and not in window order: the input
    # makes every neighbour similar, so that vectors of 6^3 to 12^3 values are summed, through every depth of numpy's recursion
    d, m = nc.one_echo_case()
    re = nc.relative_distances(d, m)
    counts = {(x1.stop - x1.start) * (y1.stop - y1.start) * (z1.stop - z1.start)
              for x1, y1, z1 in (nc.window(nc.ONE_ECHO_SHAPE, *v) for v in np.ndindex(*nc.ONE_ECHO_SHAPE))}
    assert min(counts) == 216 and max(counts) == 1728 and any(128 < c <= 256 for c in counts) and any(1024 < c for c in counts)
    want = oracle.nesma(d, m.astype(float), nthreads=8)
    assert np.array_equal(want, nc.nesma_numpy(d, m)) and not want[3, 4, 5].any()
    # nearly every pair is similar: one in a thousand is not (those with the masked-out voxel, RE = 100, and a few of the noise's tails)
    assert 0 < np.sum(re >= nc.THRESHOLD) < 1e-3 * re.size
    # and the order matters: added in window order, the values of a window give other bits than numpy's pairwise sum
    wins = [d[nc.window(nc.ONE_ECHO_SHAPE, *v)].reshape(-1) for v in np.ndindex(*nc.ONE_ECHO_SHAPE)]
    differ = sum(bool(np.add.accumulate(w)[-1] != np.sum(w)) for w in wins)
    print("MEASURED nesma one echo: the window-order sum differs from numpy's in %d of %d windows" % (differ, len(wins)))
    assert differ > 0


def test_sign_and_nonfinite_inputs_on_the_cpu(oracle):
    d = nc.negative_case()
    assert d.shape == (3, 4, 5, 9) and np.all(d < 0)
    ones = np.ones(d.shape[:3])
    assert np.all(nc.relative_distances(d, ones) <= 0)                                   # every neighbour is similar
    assert np.array_equal(oracle.nesma(d, ones), nc.window_mean(d))
    d = nc.zero_sum_case()
    assert d.shape == (2, 2, 3, 8) and np.all(d.sum(axis=-1) == 0) and np.all(d[..., 0] >= 1)
    assert np.all(np.isnan(oracle.nesma(d, np.ones(d.shape[:3]))))
    d, m = nc.nonfinite_case()
    assert d.shape == nc.SHAPE_TIES + (32,)
    for v, val in nc.NONFINITE.items():
        assert m[v] == 1 and all(0 < c < n - 1 for c, n in zip(v, nc.SHAPE_TIES))
        assert np.sum(~np.isfinite(d[v])) == 1 and (np.isnan(val) and np.isnan(d[v]).any() or np.any(d[v] == val))
    want = oracle.nesma(d, m.astype(float))
    assert np.array_equal(want, nc.nesma_numpy(d, m), equal_nan=True)
    nan_rows = {tuple(v) for v in np.argwhere(np.isnan(want).all(axis=-1))}
    # the three voxels are similar to nothing, themselves included, and nothing is similar to them: their neighbours stay finite
    assert nan_rows == set(nc.NONFINITE) | {tuple(np.unravel_index(4 * 5 * 13 - 1, nc.SHAPE_TIES))}
    assert np.isfinite(want[~np.isnan(want).all(axis=-1)]).all()


def test_smoothing_shape_is_past_one_grid():
    assert int(np.prod(SHAPE_PAST_ONE_GRID)) == 4370600 > ONE_GRID == 4194304
    assert int(np.prod(SHAPE_PAST_ONE_GRID)) * 8 < 36e6                                  # the 35 MB volume: the largest input of this file


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    from oracle import oracle
    oracle.build()
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def motor(pkg):
    return importlib.import_module(PKG + ".motor")


def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nt", nc.CASES_A, ids=_ID_A)
def test_nesma_on_every_launch_sum_branch_and_run_length(motor, oracle, shape, nt):
    import torch
    d, m, three, zero = nc.case_a(shape, nt)
    want = want_a(oracle, shape, nt)
    dt = torch.tensor(d, device="cuda")                                                  # a copy: the shared input is read-only
    got = motor.nesma_filter(dt, m)
    assert got.is_cuda and got.dtype == torch.float64
    g = got.cpu().numpy()
    assert np.array_equal(g, want, equal_nan=True)
    assert np.all(g[three] == 0) and np.all(np.isnan(g[zero]))
    assert _same_bits(motor.nesma_filter(dt, m), got)                                    # the same input, the same bits
    gn = motor.nesma_filter(d, m)                                                        # numpy in, numpy out
    assert isinstance(gn, np.ndarray) and np.array_equal(gn, want, equal_nan=True)


@pytest.mark.gpu
def test_nesma_one_echo_sums_pairwise_as_numpy(motor, oracle):
    # found by the CPU part of this file: with one echo the reference's np.mean is a pairwise sum; 3x4x5 is the smallest volume of case A
    # on which summing in window order gave other bits (14 voxels), the 12x12x13 volume sums up to 12^3 values
    d, m, _, _ = nc.case_a((3, 4, 5), 1)
    assert np.array_equal(motor.nesma_filter(d, m), nc.nesma_numpy(d, m), equal_nan=True)
    d, m = nc.one_echo_case()
    got = motor.nesma_filter(d, m)
    assert np.array_equal(got, nc.nesma_numpy(d, m)) and np.array_equal(got, oracle.nesma(d, m.astype(float), nthreads=8))


@pytest.mark.gpu
@pytest.mark.parametrize("nt", nc.NT_TIES)
def test_nesma_tie_is_not_similar(motor, oracle, nt):
    # RE == 2.5 exactly for > 5000 of the 48 000 pairs: the quotient branch of NesmaTest::similar decides them, and '<' must stay '<'
    import torch
    d = nc.tie_case(nt).astype(np.float64)
    ones = np.ones(nc.SHAPE_TIES)
    ref, ties, _ = nc.tie_reference(nt)
    got = motor.nesma_filter(torch.as_tensor(d, device="cuda"), ones).cpu().numpy()
    assert np.array_equal(got, ref)
    assert np.array_equal(got, oracle.nesma(d, ones))


@pytest.mark.gpu
def test_nesma_negative_sum_takes_every_neighbour(motor, oracle):
    d = nc.negative_case()
    ones = np.ones(d.shape[:3])
    got = motor.nesma_filter(d, ones)
    assert np.array_equal(got, oracle.nesma(d, ones))
    assert np.array_equal(got, nc.window_mean(d))


@pytest.mark.gpu
def test_nesma_zero_sum_of_nonzero_echoes_is_nan(motor, oracle):
    d = nc.zero_sum_case()
    got = motor.nesma_filter(d, np.ones(d.shape[:3]))
    assert np.all(np.isnan(got))
    assert np.array_equal(got, oracle.nesma(d, np.ones(d.shape[:3])), equal_nan=True)


@pytest.mark.gpu
def test_nesma_nonfinite_echoes(motor, oracle):
    d, m = nc.nonfinite_case()
    want = oracle.nesma(d, m.astype(float))
    got = motor.nesma_filter(d, m)
    assert np.array_equal(got, want, equal_nan=True)
    near = np.zeros(nc.SHAPE_TIES, dtype=bool)
    for v in nc.NONFINITE:
        assert np.all(np.isnan(got[v]))
        near[nc.window(nc.SHAPE_TIES, *v)] = True
        near[tuple(slice(max(c - nc.HW + 1, 0), c + nc.HW + 1) for c in v)] = True       # the voxels whose window holds v
    assert np.array_equal(np.isnan(got[near]), np.isnan(want[near])) and np.array_equal(np.isinf(got[near]), np.isinf(want[near]))


def _scipy_smooth(d, sigma):
    import scipy.ndimage as filt
    return np.stack([filt.gaussian_filter(d[..., c], sigma, 0) for c in range(d.shape[-1])], axis=-1)


@pytest.mark.gpu
def test_gaussian_smooth_past_one_grid(motor):
    # 4 370 600 elements: the threads of the capped launch (256 * 64 workgroups of 256) make a second trip through the grid-stride loop
    import torch
    d = np.random.default_rng(41).standard_normal(SHAPE_PAST_ONE_GRID)
    got = motor.gaussian_smooth(torch.as_tensor(d, device="cuda"), 2.0)
    assert np.array_equal(got.cpu().numpy(), _scipy_smooth(d, 2.0))


def _smooth_entry(pkg, shape, radius, w, data, out, work, stream=0):
    """met2_smooth_separable itself -> its return code"""
    lib = importlib.import_module(PKG + "._lib")
    w = np.ascontiguousarray(w, dtype=np.float64)
    ptr = lambda t: None if t is None else t.data_ptr()
    return lib.lib().met2_smooth_separable(0, *shape, radius, w.ctypes.data_as(C.POINTER(C.c_double)), ptr(data), ptr(out), ptr(work), stream)


@pytest.mark.gpu
def test_smooth_separable_without_a_work_array(pkg, oracle):
    # work = NULL: the entry allocates, waits for the stream and frees.  On a stream that the copy back does not wait for, so that the
    # output has to be complete when the entry returns
    import torch
    radius, w = oracle.gaussian_kernel1d(2.0)
    d = np.random.default_rng(43).standard_normal(SHAPE_NO_WORK)
    dt = torch.as_tensor(d, device="cuda")
    with_work = torch.full_like(dt, -7.0)
    assert _smooth_entry(pkg, SHAPE_NO_WORK, radius, w, dt, with_work, torch.empty_like(dt)) == 0
    without = torch.full_like(dt, -7.0)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert _smooth_entry(pkg, SHAPE_NO_WORK, radius, w, dt, without, None, side.cuda_stream) == 0
    host = torch.empty(SHAPE_NO_WORK, dtype=torch.float64).pin_memory()
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        host.copy_(without, non_blocking=True)
    other.synchronize()
    torch.cuda.synchronize()
    ref = _scipy_smooth(d, 2.0)
    assert np.array_equal(host.numpy(), ref)
    assert np.array_equal(with_work.cpu().numpy(), ref) and _same_bits(with_work, without)


@pytest.mark.gpu
def test_smooth_separable_refusals_leave_the_output_untouched(pkg, oracle):
    import torch
    shape = (5, 6, 7, 3)
    radius, w = oracle.gaussian_kernel1d(2.0)
    d = torch.as_tensor(np.random.default_rng(44).standard_normal(shape), device="cuda")
    d0 = d.clone()
    out = torch.full_like(d, -7.0)
    work = torch.full_like(d, -9.0)
    w33 = np.full(67, 1.0 / 67)
    nt0 = shape[:3] + (0,)
    for what, rc, args in [("data == out", -1, (shape, radius, w, d, d, work)),
                           ("work == out", -1, (shape, radius, w, d, out, out)),
                           ("radius 33", -2, (shape, 33, w33, d, out, work)),
                           ("nt = 0", -1, (nt0, radius, w, d, out, work))]:
        assert _smooth_entry(pkg, *args) == rc, what
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((work == -9.0).all()) and torch.equal(d, d0), what
    assert _smooth_entry(pkg, shape, radius, w, d, out, work) == 0                      # and the same arguments, put right, run
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _scipy_smooth(d0.cpu().numpy(), 2.0))


# ------------------------------------------------------------------ the earlier tests of the two filters (from test_gpu_methods.py)
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(20, 17, 15, 32), (7, 30, 9, 48), (14, 5, 13, 100), (3, 2, 2, 5), (1, 1, 1, 32)])
def test_nesma_vs_oracle(pkg, shape):
    # ragged volumes, echo counts on both kernel variants (<= 64 and <= 128), partial masks, an all-zero voxel
    import torch
    from oracle import oracle
    motor = importlib.import_module(PKG + ".motor")
    rng = np.random.default_rng(sum(shape))
    nx, ny, nz, nt = shape
    base = rng.uniform(0.5, 2.0, size=(2, nt)) * np.exp(-np.arange(nt) / 12.0)
    lab = rng.integers(0, 2, size=(nx, ny, nz))
    d = base[lab] * (1.0 + 0.01 * rng.standard_normal((nx, ny, nz, nt)))
    m = (rng.uniform(size=(nx, ny, nz)) > 0.2).astype(np.int64)
    if nx > 2:
        m[2, 0, 0] = 1; d[2, 0, 0] = 0.0                         # no similar voxel -> nan row
        m[1, 1, 1] = 3                                           # only mask == 1 is filtered
    d = d * m[..., None]
    want = oracle.nesma(d, m.astype(float), nthreads=8)
    got = motor.nesma_filter(torch.as_tensor(d, device="cuda"), m)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want, equal_nan=True)
    if nx > 2:
        assert np.all(np.isnan(want[2, 0, 0])) and np.all(want[1, 1, 1] == 0)


@pytest.mark.gpu
def test_nesma_errors(pkg):
    import torch
    motor = importlib.import_module(PKG + ".motor")
    with pytest.raises(ValueError):
        motor.nesma_filter(np.zeros((4, 4, 4)), np.ones((4, 4, 4)))
    with pytest.raises(pkg.Met2Error):
        motor.nesma_filter(np.zeros((2, 2, 2, 129)), np.ones((2, 2, 2)))
    assert motor.nesma_filter(np.zeros((0, 3, 3, 8)), np.ones((0, 3, 3))).shape == (0, 3, 3, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma,radius", [(0.5, 2), (1.0, 4), (3.3, 13), (8.0, 32)])
def test_gaussian_smooth_other_radii(pkg, sigma, radius):
    # the bit identity with scipy.ndimage.gaussian_filter at radii other than the driver's 8, up to the entry's cap of 32, on axes far
    # shorter than the radius ('reflect' folds several times: length 1, 2, 3, 5), just longer than it (33) and long (70); 1 and 63 echoes
    import torch
    import scipy.ndimage as filt
    from oracle import oracle
    motor = importlib.import_module(PKG + ".motor")
    assert oracle.gaussian_kernel1d(sigma)[0] == radius
    rng = np.random.default_rng(int(sigma * 10))
    for shp in [(1, 2, 3, 1), (5, 1, 2, 63), (3, 5, 33, 1), (33, 3, 5, 63), (2, 70, 1, 1), (70, 5, 3, 63), (5, 33, 70, 1)]:
        d = rng.standard_normal(shp)
        ref = np.stack([filt.gaussian_filter(d[..., c], sigma, 0) for c in range(shp[-1])], axis=-1)
        got = motor.gaussian_smooth(torch.as_tensor(d, device="cuda"), sigma)
        assert np.array_equal(got.cpu().numpy(), ref), (sigma, shp)
        assert np.array_equal(motor.gaussian_smooth(d, sigma), ref), (sigma, shp)            # numpy in, numpy out
