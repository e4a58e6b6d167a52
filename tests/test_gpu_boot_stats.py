"""GPU tests of the bootstrap's two statistics kernels on series handed to them directly (met2_bootstrap_series_stats ->
bootstrap_stats_kernel, met2_bootstrap_spectrum_stats -> bootstrap_spec_stats_kernel; both through series_stats): a fit never produces ties,
sorted runs, a constant with one outlier, a real nan next to the nan padding, -0.0 or a large offset with a small spread, so the kernels'
contract -- quantiles bit-equal to np.quantile, mean and std within check_stats' tolerances, both kernels the same bits -- is asserted
here on such series, over the sort sizes (every side of every power of two up to 1024) and the tile widths of the spectrum kernel.
Reference: long double for mean and std, np.quantile (method 'linear') on float64 for the quantiles.  Nonzero magnitudes stay within
[1e-150, 1e150], the domain include/met2_hip.h states."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
QP = [0.025, 0.5, 0.975]
N_REPS = [2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024]
N_REPS_INTEGER_ABSCISSA = [3, 5, 41, 81, 201, 1001]          # (n - 1) p is an integer for the median, from 41 on for p = 0.025, 0.975 too


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG).Met2Plan


# ---- the series -----------------------------------------------------------------------------------------------------------------------
def _one_off(B, at, base, other):
    v = np.full(B, base)
    v[at] = other
    return v


FAMILIES = [
    ("normal", lambda B, r: r.standard_normal(B)),
    ("offset 1e8, spread 1e-4", lambda B, r: 1e8 + 1e-4 * r.standard_normal(B)),
    ("24 decades", lambda B, r: r.standard_normal(B) * 10.0 ** r.integers(-12, 13, B)),
    ("90 % zeros", lambda B, r: np.where(r.random(B) < 0.9, 0.0, r.random(B))),
    ("one tiny then equal large", lambda B, r: _one_off(B, 0, 1e9, 1e-9)),
    ("alternating +-1e15 plus noise", lambda B, r: np.tile([1e15, -1e15], B)[:B] + r.random(B)),
    ("sorted", lambda B, r: np.sort(r.standard_normal(B))),
    ("reverse-sorted", lambda B, r: np.sort(r.standard_normal(B))[::-1].copy()),
    ("all equal", lambda B, r: np.full(B, 3.7)),
    ("all equal but the first", lambda B, r: _one_off(B, 0, 0.1, 0.3)),
    ("all equal but the last", lambda B, r: _one_off(B, B - 1, 0.1, -0.3)),
    ("all equal but the middle", lambda B, r: _one_off(B, B // 2, 1.0 / 3.0, 2.0 / 3.0)),
    ("two values, many ties", lambda B, r: np.where(r.random(B) < 0.5, 0.1, 0.7)),
    ("all -0.0", lambda B, r: np.full(B, -0.0)),
    ("-0.0 and +0.0", lambda B, r: np.where(r.random(B) < 0.5, -0.0, 0.0)),
    ("few integers (an FA index)", lambda B, r: r.integers(40, 45, B).astype(np.float64)),
    ("all equal and negative", lambda B, r: np.full(B, -1e-3)),
    ("thirds, the lerp rounds", lambda B, r: r.integers(1, 1000, B) / 3.0),
    ("all +0.0", lambda B, r: np.zeros(B)),
    ("normal at 1e150", lambda B, r: 1e150 * r.random(B)),
    ("normal at 1e-150", lambda B, r: 1e-150 * r.standard_normal(B)),
]


def make_series(B, count, seed, first=0):
    """[count, B]: the families in turn (neighbouring series come from different families), family `first` at series 0"""
    r = np.random.default_rng(seed)
    out = np.empty((count, B))
    for i in range(count):
        out[i] = FAMILIES[(first + i) % len(FAMILIES)][1](B, r)
    return out


# ---- the contract ---------------------------------------------------------------------------------------------------------------------
def reference(vals):
    """[..., n] float64 -> (mean, std with ddof 1) in long double, np.quantile [3, ...] on float64"""
    L = vals.astype(np.longdouble)
    n = vals.shape[-1]
    m = L.sum(-1) / n
    sd = np.sqrt(((L - m[..., None]) ** 2).sum(-1) / (n - 1))
    return m, sd, np.quantile(vals, QP, axis=-1, method="linear")


def check(got, vals, what):
    """got [5, ...] of vals [..., n]: check_stats of test_gpu_bootstrap_fa.py (same three assertions, same tolerances) with the long-double
    reference for mean and std"""
    assert got.shape == (5,) + vals.shape[:-1], (what, got.shape, vals.shape)
    m, sd, q = reference(vals)
    scale = np.abs(vals).max(-1)
    dm = np.abs(got[0] - m)
    ds = np.abs(got[1] - sd)
    nz = np.maximum(scale, 1e-300)
    print("%s: max |mean diff| / (1e-14 scale) = %.3g, max |std diff| / (1e-12 std + 1e-14 scale) = %.3g, quantiles equal = %s"
          % (what, float(np.max(dm / (1e-14 * nz))), float(np.max(ds / (1e-12 * sd + 1e-14 * nz))), np.array_equal(got[2:], q)))
    assert np.array_equal(got[2:], q), what                                   # quantiles bit-equal to np.quantile
    assert np.all(dm <= 1e-14 * scale), what
    assert np.all(ds <= 1e-12 * sd + 1e-14 * scale), what


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def series_stats(P, series, status=None):
    """[N, B] with N a multiple of 8, as 8 quantities of N / 8 voxels -> [5, N]"""
    N, B = series.shape
    got = P.bootstrap_series_stats(dev(series.reshape(8, N // 8, B)), status).cpu().numpy()       # [8, 5, N / 8]
    return np.moveaxis(got, 1, 0).reshape(5, N)


def spectrum_stats(P, series, nt2, status=None):
    """[N, B] with N = nvox nt2, series v nt2 + j as bin j of voxel v -> [5, N]"""
    N, B = series.shape
    fsol_r = series.reshape(N // nt2, nt2, B).transpose(0, 2, 1)                                  # [nvox, B, nt2]
    return P.bootstrap_spectrum_stats(dev(fsol_r), status).cpu().numpy().reshape(5, N)


# ---- series statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", N_REPS)
def test_series_stats_against_numpy(P, B):
    series = make_series(B, 8 * len(FAMILIES), seed=1000 + B)
    check(series_stats(P, series), series, "series n_rep=%d" % B)
    nq3 = P.bootstrap_series_stats(dev(series[:12].reshape(3, 4, B))).cpu().numpy()               # n_quant = 3: no reg row, no FA row
    check(np.moveaxis(nq3, 1, 0).reshape(5, 12), series[:12], "series n_rep=%d, 3 quantities" % B)
    one = P.bootstrap_series_stats(dev(series[:5])).cpu().numpy()                                 # [nvox, n_rep] -> [5, nvox]
    check(one, series[:5], "series n_rep=%d, 1 quantity" % B)


def _lerp_branch_matters(series, p):
    """does numpy's t >= 0.5 branch change a bit of the p-quantile of some series?  (a + d g against b - d (1 - g))"""
    s = np.sort(series, axis=-1)
    n = s.shape[-1]
    h = (n - 1) * p
    i0 = int(np.floor(h))
    g = h - i0
    if g < 0.5 or i0 + 1 >= n:
        return False
    a, b = s[:, i0], s[:, i0 + 1]
    d = b - a
    return bool(np.any(a + d * g != b - d * (1.0 - g)))


@pytest.mark.parametrize("B", N_REPS_INTEGER_ABSCISSA)
def test_quantile_abscissa_on_an_integer(P, B):
    for p in QP if B >= 41 else [0.5]:
        h = (B - 1) * p
        assert h == np.floor(h), (B, p)                                       # the premise: h is an integer in float64, as the kernel forms it
    series = make_series(B, 8 * len(FAMILIES), seed=2000 + B)
    check(series_stats(P, series), series, "integer abscissa n_rep=%d" % B)
    check(spectrum_stats(P, series, 12), series, "integer abscissa n_rep=%d, spectrum kernel" % B)


@pytest.mark.parametrize("B", [4, 33, 64, 100, 1000, 1024])
def test_the_lerp_branch_changes_a_bit_and_the_kernels_follow_numpy(P, B):
    series = make_series(B, 8 * len(FAMILIES), seed=3000 + B)
    assert any(_lerp_branch_matters(series, p) for p in QP), B               # without this the test could not see a dropped branch
    check(series_stats(P, series), series, "lerp branch n_rep=%d" % B)
    check(spectrum_stats(P, series, 8), series, "lerp branch n_rep=%d, spectrum kernel" % B)


@pytest.mark.parametrize("B", [3, 33, 63, 100, 1000])
def test_a_real_nan_next_to_the_nan_padding(P, B):
    assert B & (B - 1) != 0                                                   # not a power of two: the sort pads with nan
    series = make_series(B, 24, seed=4000 + B)
    hit = {1: 0, 10: B // 2, 20: B - 1}                                       # series -> where its nan sits
    for i, at in hit.items():
        series[i, at] = np.nan
    clean = np.array([i for i in range(24) if i not in hit])
    for what, got in (("series", series_stats(P, series)), ("spectrum", spectrum_stats(P, series, 12))):
        assert np.all(np.isnan(got[:, list(hit)])), what                      # all five, as numpy
        check(got[:, clean], series[clean], "%s kernel, neighbours of a nan series, n_rep=%d" % (what, B))


@pytest.mark.parametrize("B", [2, 5, 64, 100, 1024])
def test_negative_zero(P, B):
    r = np.random.default_rng(B)
    series = np.stack([np.full(B, -0.0), np.where(r.random(B) < 0.5, -0.0, 0.0), _one_off(B, B - 1, -0.0, 0.0), _one_off(B, 0, 0.0, -0.0),
                       np.zeros(B), np.full(B, -0.0), r.standard_normal(B), np.full(B, -0.0)])
    want = np.concatenate([series.mean(-1)[None], series.std(-1, ddof=1)[None], np.quantile(series, QP, axis=-1)], 0)
    for what, got in (("series", series_stats(P, series)), ("spectrum", spectrum_stats(P, series, 8))):
        assert np.all(got[:, [0, 1, 2, 3, 4, 5, 7]] == 0.0), what
        assert np.array_equal(got[2:], want[2:]) and np.array_equal(got[:2, :6], want[:2, :6]), what       # numpy's values under ==
        check(got, series, "%s kernel, zeros of both signs, n_rep=%d" % (what, B))


# ---- both kernels, the same bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", N_REPS)
def test_both_kernels_give_the_same_bits(P, B):
    """The same series as a quantity of bootstrap_stats_kernel (the long way, always) and as a bin column of bootstrap_spec_stats_kernel
    (whose series_stats may take the shortcut for constant series): constant series, constant -0.0 (which the shortcut must leave to the
    long way: its sums give +0.0) and a series with a nan included."""
    series = make_series(B, 240, seed=5000 + B)
    names = [FAMILIES[i % len(FAMILIES)][0] for i in range(240)]
    assert "all equal" in names and "all -0.0" in names and "all +0.0" in names
    series[7, B // 2] = np.nan
    a = series_stats(P, series)
    b = spectrum_stats(P, series, 60)
    assert np.all(np.isnan(a[:, 7])) and np.all(np.isnan(b[:, 7]))
    keep = np.arange(240) != 7
    for s, name in enumerate(("mean", "std", "q025", "q500", "q975")):
        bad = np.where(a[s].view(np.int64)[keep] != b[s].view(np.int64)[keep])[0]
        assert bad.size == 0, (name, [names[i + (i >= 7)] for i in bad[:5]])
    check(a[:, keep], series[keep], "both kernels n_rep=%d" % B)


# ---- the spectrum kernel's tiles ----------------------------------------------------------------------------------------------------------
SPEC_NT2 = [1, 12, 60, 63, 64, 65, 120, 127, 128]
SPEC_NREP = [(2, 64), (33, 64), (64, 64), (65, 32), (128, 32), (512, 8), (1024, 4)]        # n_rep, bins per tile


def test_spectrum_launch_geometry(P):
    """the premise of the sweep below, from the library's own helper: these n_rep give tiles of 64, 64, 64, 32, 32, 8 and 4 bins, both padding
    rules, and a dynamic LDS request within the 64 KiB a kernel gets"""
    pads = set()
    for B, w_want in SPEC_NREP:
        w, S, lds = P.bootstrap_spec_launch_info(B)
        Pw = 1 << (B - 1).bit_length()
        assert w == w_want and lds == 8 * (w * S + 5 * w) and 0 < lds <= 65536, (B, w, S, lds)
        assert S >= Pw and w * S * 8 <= lds
        pads.add(S - Pw)
        for nt2 in SPEC_NT2:
            assert (nt2 % w == 0) == ((nt2, w) in ((64, 64), (128, 64), (64, 32), (128, 32), (64, 8), (120, 8), (128, 8), (12, 4), (60, 4), (64, 4),
                                                   (120, 4), (128, 4)))
    assert pads == {1, 2, 4}
    for B in range(2, 1025):
        assert P.bootstrap_spec_launch_info(B)[2] <= 65536, B


@pytest.mark.parametrize("nt2", SPEC_NT2)
@pytest.mark.parametrize("B,w", SPEC_NREP)
def test_spectrum_stats_tiles(P, B, w, nt2):
    """Every bin column a series of its own, neighbouring bins from different families, so a transposed index or a tile offset puts a result
    into a wrong bin; three voxels with the middle one gated: it gets zeros (its values, all nan, are not read) and its neighbours are
    exact.  The same series through the other kernel: the same bits."""
    nvox = 3
    series = make_series(B, nvox * nt2, seed=6000 + 7 * B + nt2, first=(B + nt2) % len(FAMILIES))
    series[nt2:2 * nt2] = np.nan
    status = np.array([1, 0, 3], dtype=np.int32)                              # 3: a fitted voxel with another bit set
    got = spectrum_stats(P, series, nt2, status).reshape(5, nvox, nt2)
    assert np.all(got[:, 1] == 0.0)
    live = np.r_[0:nt2, 2 * nt2:3 * nt2]
    check(got.reshape(5, -1)[:, live], series[live], "spectrum n_rep=%d nt2=%d (tiles of %d)" % (B, nt2, w))
    pad = (-len(live)) % 8
    both = np.concatenate([series[live], make_series(B, pad, seed=1)], 0)
    other = series_stats(P, both)[:, :len(live)]
    assert same_bits(other, got.reshape(5, -1)[:, live])
    # status = None takes every voxel
    series[nt2:2 * nt2] = make_series(B, nt2, seed=2)
    everyone = spectrum_stats(P, series, nt2).reshape(5, nvox, nt2)
    assert same_bits(everyone[:, [0, 2]], got[:, [0, 2]])
    check(everyone[:, 1], series[nt2:2 * nt2], "spectrum n_rep=%d nt2=%d, no status" % (B, nt2))


def test_series_stats_gating(P):
    B, nvox = 100, 5
    series = make_series(B, 8 * nvox, seed=77).reshape(8, nvox, B)
    series[:, 1] = np.nan
    series[:, 4] = np.nan
    status = np.array([1, 0, 1, 17, 2], dtype=np.int32)                       # 2: bits set, but not MET2_ST_FITTED
    got = P.bootstrap_series_stats(dev(series), status).cpu().numpy()       # [8, 5, nvox]
    assert np.all(got[:, :, [1, 4]] == 0.0)
    check(np.moveaxis(got[:, :, [0, 2, 3]], 1, 0), series[:, [0, 2, 3]], "series kernel, gated neighbours")


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [33, 512, 1000])
def test_two_calls_and_a_split_call_give_the_same_bits(P, B):
    nvox, nt2 = 7, 65
    series = make_series(B, nvox * nt2, seed=8000 + B)
    fsol_r = dev(series.reshape(nvox, nt2, B).transpose(0, 2, 1))
    status = torch.ones(nvox, dtype=torch.int32, device="cuda:0")
    one = P.bootstrap_spectrum_stats(fsol_r, status)
    assert torch.equal(one.view(torch.int64), P.bootstrap_spectrum_stats(fsol_r, status).view(torch.int64))
    parts = torch.cat([P.bootstrap_spectrum_stats(fsol_r[:3], status[:3]), P.bootstrap_spectrum_stats(fsol_r[3:], status[3:])], dim=1)
    assert torch.equal(one.view(torch.int64), parts.view(torch.int64))
    pad = (-nvox * nt2) % 8
    vals = dev(np.concatenate([series, make_series(B, pad, seed=3)], 0).reshape(8, -1, B))
    nv = vals.shape[1]
    st = torch.ones(nv, dtype=torch.int32, device="cuda:0")
    one = P.bootstrap_series_stats(vals, st)
    assert torch.equal(one.view(torch.int64), P.bootstrap_series_stats(vals, st).view(torch.int64))
    cut = nv // 3
    parts = torch.cat([P.bootstrap_series_stats(vals[:, :cut], st[:cut]), P.bootstrap_series_stats(vals[:, cut:], st[cut:])], dim=2)
    assert torch.equal(one.view(torch.int64), parts.view(torch.int64))
