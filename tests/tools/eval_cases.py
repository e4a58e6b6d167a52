"""The cases that tests/test_eval_host.py (numpy restatement against SciPy, no device) and tests/test_gpu_eval_kernels.py (the kernels of
csrc/met2_eval.hip against the restatement) share: adversarial spectra for met2_eval_voxel_metrics at every bin count where the kernel
changes path, inputs for met2_eval_reduce, and T2 grids for met2_synth_two_lobe.  numpy only.

A voxel case is (name, kind, fsol [n_t2], dist2 [n_t2]):
  'exact'    fsol holds small non-negative integers whose total is a power of two: km, x = fsol / km and every partial sum of x are exact in
             any order of summation (assert_exact_sums), so fM, fIE, km and the peak count must be EQUAL on the device
  'sort'     inputs that stress the Wasserstein distance's sort (order, ties, signs, signed zeros, NaN)
  'special'  NaN / Inf / all-zero inputs and exact zeros in dist2: the NaN pattern must be equal
  'float'    seeded sparse NNLS-like and smooth spectra for the rounding bound
"""
import math

import numpy as np

N_T2 = (3, 4, 5, 63, 64, 65, 127, 128)                             # one and two bins per lane, sort padding 4 / 8 / 64 / 128
BIG, TOTAL = 100000.0, 131072.0                                    # the threshold tie: 1e-5 * (BIG / TOTAL) == 1 / TOTAL in float64


def adversarial_spectra():
    rng = np.random.default_rng(5)
    xs = [
        np.array([0.0, 1.0, 1.0, 1.0, 0.0, 2.0, 2.0, 0.5, 0.0, 0.0]),          # plateaus
        np.array([0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]),          # a single non-zero
        np.array([5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0]),          # endpoints only: never peaks
        np.array([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]),          # a plateau that runs into the last sample
        np.array([0.0, 1e-5, 0.0, 1.0, 0.0, 0.99999e-5, 0.0, 0.0, 2e-5, 1e-5]), # ties at the height threshold 1e-5 max
        np.array([0.0, 2.0, 1.0, 2.0, 1.0, 2.0, 2.0, 1.0, 3.0, 3.0]),
    ]
    for _ in range(6):                                                         # sparse NNLS-like spectra with runs of exact zeros
        x = np.where(rng.random(60) < 0.2, rng.random(60), 0.0)
        x[rng.integers(0, 60, 3)] = 0.5                                        # exact ties
        xs.append(x)
    xs.append(np.exp(-0.5 * ((np.arange(120) - 40.0) / 6.0) ** 2))           # smooth, 120 bins
    return xs


# the six hand-written vectors above as integers with a power-of-two total and the same order relations between neighbours (0.5 -> 2 under
# a plateau of 4; one 1 -> 0; the plateau of nine ones cut to eight; the threshold ties on the exact tie BIG / TOTAL)
HAND_INT = (
    ("plateaus", [0, 2, 2, 2, 0, 4, 4, 2, 0, 0]),
    ("single", [0, 0, 0, 4, 0, 0, 0, 0, 0, 0]),
    ("endpoints", [4, 0, 0, 0, 0, 0, 0, 0, 0, 4]),
    ("plateau_to_end", [0, 0, 1, 1, 1, 1, 1, 1, 1, 1]),
    ("threshold_ties", [0, 1, 0, BIG, 0, 2, 1, 0, 31068, 0]),
    ("zigzag", [0, 2, 1, 2, 1, 2, 2, 0, 3, 3]),
)
TIE10 = [0, 0, 0, BIG, 0, 0, 1, 0, 31071, 0]                       # bin 6 sits on the threshold: a peak by hmin <= x, none by <
TIE10_TWO = [0, 0, 0, 2 * BIG, 0, 0, 2, 0, 62142, 0]               # the same tie at twice the total
TIE10_TWIN = [0, 0, 0, 2 * BIG, 0, 0, 1, 0, 62143, 0]              # ... and that bin one level lower: below the threshold, no peak
TIE5, TIE5_TWO, TIE5_TWIN = [31071, BIG, 0, 1, 0], [62142, 2 * BIG, 0, 2, 0], [62143, 2 * BIG, 0, 1, 0]


def t2_grid(n):
    """logspace(10, 2000, n) with the bins nearest 40 and 200 moved onto 40.0 and 200.0 exactly: both default cuts (<=) fall on a bin"""
    g = np.logspace(1.0, math.log10(2000.0), n)
    if n == 3:
        g = np.array([40.0, 200.0, 2000.0])
    else:
        g[np.argmin(np.abs(g - 40.0))] = 40.0
        g[np.argmin(np.abs(g - 200.0))] = 200.0
    assert np.all(np.diff(g) > 0) and 40.0 in g and 200.0 in g
    return g


def other_cuts(T2s):
    """cuts that are other bins of the grid, exactly"""
    n = T2s.shape[0]
    return float(T2s[max(0, n // 4 - 1)]), float(T2s[min(n - 1, (2 * n) // 3)])


def grid_above_ie(n):
    return np.linspace(250.0, 2000.0, n)


def is_pow2(v):
    m, e = math.frexp(v)
    return v > 0 and m == 0.5


def _pairwise(a):
    return a[0] if len(a) == 1 else _pairwise(a[:len(a) // 2]) + _pairwise(a[len(a) // 2:])


def _three_sums(a):
    fw = bw = np.float64(0.0)
    for v in a:
        fw = fw + v
    for v in a[::-1]:
        bw = bw + v
    return fw, bw, (_pairwise(list(a)) if len(a) else np.float64(0.0))


def assert_exact_sums(f, T2s, cut_m=40.0, cut_ie=200.0):
    """f: integers >= 0 with a power-of-two total -> km, x = f / km, fM, fIE sum to the same bits forwards, backwards and pairwise"""
    f = np.asarray(f, dtype=np.float64)
    assert np.all(f >= 0) and np.all(f == np.round(f)) and is_pow2(float(math.fsum(f))), f
    km = np.float64(math.fsum(f))
    x = f / km
    assert np.all(x * km == f)                                     # the division is exact
    im, it = T2s <= cut_m, (T2s > cut_m) & (T2s <= cut_ie)
    for a, want in ((f, km), (x, 1.0), (x[im], math.fsum(x[im])), (x[it], math.fsum(x[it]))):
        assert all(s == want for s in _three_sums(a)), (f, want)
    return km, x


def _place(n, off, pat):
    f = np.zeros(n)
    f[off:off + len(pat)] = pat
    return f


def _offsets(n, m):
    # first bins, last bins, and across the lane boundary: a 10-bin pattern at 58 covers 58..67, so it straddles 62..66
    return sorted({0, n - m, min(58, n - m)})


def default_dist2(n, k=0):
    """a smooth positive distribution (sum 1 up to rounding), peak position varied with k"""
    i = np.arange(n, dtype=np.float64)
    d = np.exp(-0.5 * ((i - (0.3 + 0.05 * (k % 9)) * n) / (0.15 * n + 0.5)) ** 2) + 1e-3
    if n < 10:                                                     # at so few bins a bell is close to many spectra, and a small jsd is ill-conditioned
        d = 0.3 ** ((i + k) % n) + 1e-3
    return d / d.sum()


def exact_spectra(n):
    """(name, fsol) of the 'exact' cases at n bins"""
    out = []
    if n < 10:
        # every vector over {0, 1, 2} with a power-of-two total: all plateau / endpoint / peak-at-n-2 patterns these bin counts can hold
        for c in range(1, 3 ** n):
            v = [(c // 3 ** j) % 3 for j in range(n)]
            if is_pow2(float(sum(v))):
                out.append(("enum%d" % c, np.array(v, dtype=np.float64)))
        if n == 5:                                                 # the smallest bin count that can hold the tie (3 and 4 cannot)
            out += [("tie", np.array(TIE5)), ("tie_two", np.array(TIE5_TWO)), ("tie_twin", np.array(TIE5_TWIN))]
        return out
    for name, pat in HAND_INT + (("tie", TIE10), ("tie_two", TIE10_TWO), ("tie_twin", TIE10_TWIN)):
        for off in _offsets(n, 10):
            out.append(("%s@%d" % (name, off), _place(n, off, pat)))
    out.append(("plateau_from_1", _place(n, 1, [1, 1])))
    out.append(("plateau_from_1_long", _place(n, 1, [1] * 32)))
    out.append(("plateau_into_last", _place(n, n - 8, [1] * 8)))
    out.append(("plateau_into_last_long", _place(n, n - 33, [0] + [1] * 32)))
    out.append(("peak_at_n-2", _place(n, n - 3, [0, 1, 0])))
    out.append(("peak_at_n-2_and_1", _place(n, 0, [0, 1, 0]) + _place(n, n - 3, [0, 1, 0])))
    ends = np.zeros(n)
    ends[0] = ends[n - 1] = 4.0
    out.append(("endpoints_only", ends))
    if n >= 65:                                                    # plateaus across lanes 63 | 64 (bins lane and lane + 64)
        out.append(("plateau_61..64", _place(n, 60, [0, 1, 1, 1, 1])))         # at n = 65 it runs into the last sample: no peak
    if n >= 66:
        out.append(("plateau_62..65", _place(n, 61, [0, 1, 1, 1, 1])))
        out.append(("plateau_63..64", _place(n, 62, [0, 1, 1, 0])))
        out.append(("step_up_63_64", _place(n, 62, [0, 1, 3, 0])))
        out.append(("plateau_1..64", _place(n, 1, [1] * 64)))
    return out


def sort_cases(n):
    """(name, fsol, dist2) that stress the sort of the Wasserstein distance"""
    rng = np.random.default_rng(1000 + n)
    up = np.arange(1, n + 1, dtype=np.float64)
    sq = up * up / np.sum(up * up)
    out = [("sorted", up.copy(), sq), ("reversed", up[::-1].copy(), sq), ("both_reversed", up[::-1].copy(), sq[::-1].copy()),
           ("x_all_equal", np.ones(n), rng.random(n)), ("dist2_all_equal", rng.permutation(up ** 3), np.full(n, 0.25)),
           ("ties", rng.integers(0, 4, n).astype(np.float64) + _place(n, 0, [1]), rng.integers(0, 3, n) / 8.0 + _place(n, n - 1, [0.125])),
           ("random", rng.random(n) * 1000.0, rng.random(n))]
    if is_pow2(float(n)):                                          # 1 / n is exact: x == dist2 in every precision, jsd = wd = 0
        out.append(("all_equal", np.ones(n), np.full(n, 1.0 / n)))
    f = rng.integers(-3, 9, n).astype(np.float64)
    f[0] = -2.0
    f[n - 1] = 3.0 * n                                             # a positive total whatever the draws
    out.append(("negative", f, rng.normal(size=n)))
    f = np.where(np.arange(n) % 3 == 0, -0.0, np.where(np.arange(n) % 3 == 1, 0.0, 2.0))
    f[n - 1] = 4.0
    out.append(("signed_zeros", f, np.where(np.arange(n) % 2 == 0, 0.0, -0.0) + _place(n, 1, [1.0])))
    d = rng.random(n)
    d[n // 2] = np.nan
    out.append(("nan_in_dist2", rng.random(n) * 100.0 + 1.0, d))
    return out


def special_cases(n):
    rng = np.random.default_rng(2000 + n)
    d = default_dist2(n)
    base = rng.integers(0, 5, n).astype(np.float64)
    base[n // 2] = 3.0
    out = [("all_zero", np.zeros(n), d)]
    for pos in sorted({0, n // 2, n - 1}):
        f = base.copy()
        f[pos] = np.inf
        out.append(("inf@%d" % pos, f, d))
        f = base.copy()
        f[pos] = np.nan
        out.append(("nan@%d" % pos, f, d))
    f = _place(n, 0, [0, 4, 0]) + _place(n, n - 1, [4])          # total 8
    dz = np.where(np.arange(n) % 2 == 0, 0.0, d)
    out.append(("dist2_zeros", f, dz / dz.sum()))                  # dist2 zero where x is zero (bin 0) and where it is not (n - 1 even, or 1)
    dz = np.where(f > 0, 0.0, d)
    out.append(("dist2_zero_where_x_is_not", f, dz))
    dz = np.where(f > 0, d, 0.0)
    out.append(("dist2_zero_where_x_is_zero", f, dz))
    out.append(("dist2_equals_x", f, f / 8.0))
    g = rng.integers(0, 9, n).astype(np.float64)
    g[0] += 1024.0 - g.sum()
    out.append(("dist2_equals_x_dense", g, g / 1024.0))
    return out


def float_spectra(n):
    """(name, fsol, dist2): seeded sparse NNLS-like spectra (runs of exact zeros, exact ties) and smooth ones, scaled like a first echo"""
    rng = np.random.default_rng(3000 + n)
    i = np.arange(n, dtype=np.float64)
    out = []
    for k in range(10):
        x = np.where(rng.random(n) < max(0.2, 2.0 / n), rng.random(n), 0.0)
        x[rng.integers(0, n, 2)] = 0.5
        d = default_dist2(n, k) if k % 2 else np.where(rng.random(n) < 0.3, 0.0, rng.random(n)) + _place(n, n // 2, [0.25])
        out.append(("sparse%d" % k, x * (500.0 + 100.0 * k), d / d.sum()))
    for k in range(4):
        x = np.exp(-0.5 * ((i - 0.3 * n - k) / (0.05 * n + 0.7)) ** 2) + 0.6 * np.exp(-0.5 * ((i - 0.7 * n + k) / (0.08 * n + 0.7)) ** 2)
        d = np.exp(-i / (0.12 * n + 0.4 + 0.1 * k)) + 1e-3          # far from x: a small jsd is a difference of nearly equal sums
        out.append(("smooth%d" % k, x * 1000.0, d / d.sum()))
    return out


def voxel_cases(n):
    """all cases at n bins in launch order, the special ones spread between the others: (name, kind, fsol, dist2)"""
    plain = [(nm, "exact", f, default_dist2(n, k)) for k, (nm, f) in enumerate(exact_spectra(n))]
    plain += [(nm, "sort", f, d) for nm, f, d in sort_cases(n)]
    plain += [(nm, "float", f, d) for nm, f, d in float_spectra(n)]
    special = [(nm, "special", f, d) for nm, f, d in special_cases(n)]
    out, step = [], max(1, len(plain) // (len(special) + 1))
    for k, c in enumerate(plain):
        out.append(c)
        if (k + 1) % step == 0 and special:
            out.append(special.pop(0))
    return out + special


def has_nonfinite(c):
    return not (np.all(np.isfinite(c[2])) and np.all(np.isfinite(c[3])))


# ---------------------------------------------------------------- met2_eval_reduce

REDUCE_N = (1, 2, 255, 256, 257, 4099)                             # 256 threads: one partial wave, one voxel each, one voxel more, many passes


def reduce_inputs(n, seed=3):
    """per-voxel rows, truth rows, lambda and an NNLS fIE array built like test_aggregates_match_the_reference_formulas"""
    rng = np.random.default_rng(seed + n)
    T = rng.uniform(0.05, 0.25, n)
    truth = np.stack([T, rng.uniform(15, 35, n), rng.uniform(60, 90, n), np.full(n, 1000.0), rng.uniform(90, 180, n), rng.uniform(50, 150, n),
                      rng.uniform(0.05, 0.25, n), rng.uniform(1, 3, n), rng.uniform(6, 12, n)])
    pv = np.stack([T + rng.normal(0, 0.03, n), 1 - T + rng.normal(0, 0.03, n), truth[1] * rng.uniform(0.8, 1.2, n), truth[2] * rng.uniform(0.9, 1.1, n),
                   1000 * rng.uniform(0.95, 1.05, n), rng.integers(1, 5, n).astype(float), rng.random(n) * 0.02, rng.random(n), rng.random(n) * 0.01])
    lam = rng.lognormal(-3, 2, n)
    fie = 1 - T + rng.normal(0, 0.05, n)
    return pv, truth, lam, fie


def degenerate_reduce_inputs(nan_column):
    """name -> (pv, truth, lam, fie): columns on which an aggregate is 0/0, x/0 or NaN.  The constants are dyadic, so their means and the
    deviations from them are exact zeros in every precision and summation order.  nan_column: the 9 per-voxel values of an all-zero fit."""
    out = {}
    for n in (2, 257):
        pv, truth, lam, fie = reduce_inputs(n, seed=40)
        a = pv.copy(); a[0] = 0.125
        out["constant_M_n%d" % n] = (a, truth, lam, fie)
        t = truth.copy(); t[0] = 0.25
        out["constant_T_n%d" % n] = (pv, t, lam, fie)
        out["constant_M_and_T_n%d" % n] = (a, t, lam, fie)
        t = truth.copy(); t[0, n // 2] = 0.0
        out["T_is_0_n%d" % n] = (pv, t, lam, fie)
        a0 = pv.copy(); a0[0, n // 2] = 0.0
        out["T_and_M_are_0_n%d" % n] = (a0, t, lam, fie)
        t = truth.copy(); t[0, n - 1] = 1.0
        out["T_is_1_n%d" % n] = (pv, t, lam, fie)
        a = pv.copy(); a[:, n - 1] = nan_column
        out["nan_voxel_n%d" % n] = (a, truth, lam, fie)
    pv, truth, lam, fie = reduce_inputs(1, seed=40)
    out["n1"] = (pv, truth, lam, fie)
    return out


# ---------------------------------------------------------------- met2_synth_two_lobe

def midpoint_grid():
    """A T2 grid with one bin edge exactly on a point g of linspace(1, 300, 1000): T2s[i-1] = g - d, T2s[i] = g + d with dyadic d, chosen so
    that the midpoint expression returns g bit for bit.  -> (T2s, i, index of g in the fine grid)"""
    fine = np.linspace(1.0, 300.0, 1000)
    d = 0.5
    for j in range(240, 260):                                      # near 75 ms, inside the intermediate lobe: the point carries weight
        g = fine[j]
        lo, hi = g - d, g + d
        if lo + (hi - lo) / 2.0 == g and (lo + d == g) and (hi - d == g):
            T2s = np.array([10.0, 20.0, 40.0, lo, hi, 120.0, 200.0, 2000.0])
            assert np.all(np.diff(T2s) > 0)
            return T2s, 4, j
    raise AssertionError("no grid point near 75 ms has an exact midpoint")


# ---------------------------------------------------------------- comparing with a long-double reference

def rel_err(got, want):
    """max over elements of |got - want| / |want|, in long double.  Where want is NaN or Inf, got must be the same NaN or Inf; where want is
    0, got must be 0: anything else counts as an infinite error."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.longdouble)), np.atleast_1d(np.asarray(want, dtype=np.longdouble))
    assert got.shape == want.shape
    fin = np.isfinite(want)
    same = np.where(np.isnan(want), np.isnan(got), got == want)
    if not np.all(same[~fin]) or not np.all(same[fin & (want == 0)]):
        return float("inf")
    nz = fin & (want != 0)
    if not np.any(nz):
        return 0.0
    if not np.all(np.isfinite(got[nz])):
        return float("inf")
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))
