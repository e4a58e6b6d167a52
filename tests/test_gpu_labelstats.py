"""GPU tests of met2_label_stats and its stage entries (csrc/met2_stats.hip), motor.label_stats_filter and tissue_stats='yes' in the drivers,
against the numpy restatement (tests/tools/labelstats_numpy.py, which follows include/met2_hip.h).

Index: order and offset EQUAL the restatement's (a stable sort has one answer); member counts 0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1,
2 CHUNK + 1 and 65 537 with 1, 3 and 257 labels, some empty; the labels -1 and n_label among the voxels; members scattered at random.
Moments: n exact; |mean - ref| <= 1e-13 max|v| and |std - ref| <= 1e-12 std + 1e-13 max|v| against long double -- no chain of additions is
longer than 512 terms and 512 * 2^-53 = 5.7e-14.  Both layouts; 1, 8, 60, 128 and 129 series; NaNs among the members of one series.
Quantiles: EQUAL (==) to np.quantile of the installed numpy for q = 0, 0.025, 0.25, 1/3, 0.5, 0.75, 0.975, 1; n = 1, 2, 3, SMALL_N - 1,
SMALL_N, SMALL_N + 1, CHUNK - 1, CHUNK + 1 and 65 537; the value patterns of labelstats_numpy.PATTERNS.  Order statistics are exact, so the
equality needs no margin.  Permuting the voxels and running twice change no bit.
The whole entry equals the stages; the limits and return codes hold with nothing written.
Drivers: res['tissue_stats'] equals the restatement applied to the same run's own arrays and labels (TWC_seg / TWC_pve of that run, not a
second segmentation); the other outputs are bit-equal to the run without tissue_stats; the tables read back to the dict.
Measured figures: profiles/labelstats_parity.json."""
import ctypes
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
import labelstats_numpy as ln                                      # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
CHUNK, SMALL_N = ln.CHUNK, ln.SMALL_N
EDGE_COUNTS = (0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 65537)


def record(name, figures):
    """with MET2_LABELSTATS_PARITY_JSON set, the measured deviations are kept in that file (profiles/labelstats_parity.json was written so)"""
    path = os.environ.get("MET2_LABELSTATS_PARITY_JSON")
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


@pytest.fixture(scope="module")
def stats(motor):
    return importlib.import_module(PKG + ".stats")


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- index

def index_counts(name):
    rng = np.random.default_rng(11)
    if name == "L1":
        return [65537], 100000
    if name == "L3":
        return [CHUNK + 1, 0, 2], 40000
    if name == "L3_empty":
        return [0, 0, 0], 1000
    counts = rng.integers(0, 40, 257)
    counts[rng.permutation(257)[:40]] = 0
    counts[[256, 5, 100, 17, 0, 200, 33, 128]] = EDGE_COUNTS
    return [int(c) for c in counts], 2 ** 18


@functools.lru_cache(maxsize=None)
def index_case(name):
    counts, nvox = index_counts(name)
    lab = ln.scatter_labels(np.random.default_rng(12), nvox, counts)
    offset, order = ln.member_list(lab, len(counts))
    return frozen(lab, offset, order) + (counts,)


def test_the_cases_hold_the_edges():
    counts, nvox = index_counts("L257")
    assert len(counts) == 257 and all(c in counts for c in EDGE_COUNTS) and sum(counts) < nvox <= 2 ** 18
    lab = index_case("L257")[0]
    assert (lab == -1).any() and (lab == 257).any()
    assert CHUNK == 16384 and SMALL_N == 1024


@pytest.mark.parametrize("name", ["L1", "L3", "L3_empty", "L257"])
def test_index_equals_the_stable_sort(stats, name):
    lab, offset, order, counts = index_case(name)
    got_offset, got_order = stats.label_index(lab, len(counts))
    assert got_offset.dtype == np.int32 and np.array_equal(got_offset, offset) and np.diff(got_offset).tolist() == counts
    assert np.array_equal(got_order, order)
    again = stats.label_index(torch.as_tensor(lab, device="cuda"), len(counts))
    assert np.array_equal(again[0], offset) and np.array_equal(again[1], order)


def test_index_of_no_voxel(stats):
    offset, order = stats.label_index(np.zeros(0, dtype=np.int32), 4)
    assert offset.tolist() == [0] * 5 and order.size == 0


# ---- moments

MOMENT_CASES = {                                                   # counts per label, voxels, series, layout
    "L257_S1_series": (None, None, 1, "series"),
    "L3_S8_series": ([CHUNK - 1, 0, 2 * CHUNK + 1], 60000, 8, "series"),
    "L3_S8_voxel": ([CHUNK, 1, CHUNK + 1], 40000, 8, "voxel"),
    "L3_S1_voxel": ([2, CHUNK + 1, 3], 20000, 1, "voxel"),
    "L3_S60_voxel": ([CHUNK, CHUNK + 1, 1], 40000, 60, "voxel"),
    "L1_S128_voxel": ([CHUNK + 1], 20000, 128, "voxel"),
    "L3_S129_series": ([2, CHUNK + 1, 0], 20000, 129, "series"),
    "L2_S129_voxel": ([300, CHUNK - 1], 20000, 129, "voxel"),
}


@functools.lru_cache(maxsize=None)
def moment_case(name):
    counts, nvox, S, layout = MOMENT_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if counts is None:
        lab, offset, order, counts = index_case("L257")
        nvox = lab.size
    else:
        lab = ln.scatter_labels(rng, nvox, counts)
        offset, order = ln.member_list(lab, len(counts))
    v = 100.0 + 10.0 * rng.standard_normal((S, nvox))
    s_nan = S // 2
    v[s_nan, rng.random(nvox) < 0.02] = np.nan                      # NaNs in one series: skipped, n reduced for that series only
    if S > 2:
        v[S - 1, order[offset[0]:offset[1]]] = np.nan               # and a (label, series) without a value
    if layout == "voxel":
        v = np.ascontiguousarray(v.T)
    ref = ln.moments(v, offset, order, layout)
    return frozen(v, np.array(lab), np.array(offset), np.array(order), ref) + (layout, s_nan)


def check_moments(got, ref, v, name, layout="series"):
    """n exact, mean and std within the header's bounds of the long-double restatement, max|v| taken per series -> the measured figures"""
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(got[..., 0], ref[..., 0].astype(np.float64))
    empty = ref[..., 0] == 0
    assert np.isnan(got[empty][:, 1:]).all() and not np.isnan(got[~empty][:, 1]).any()
    assert np.array_equal(np.isnan(got[..., 2]), np.isnan(ref[..., 2].astype(np.float64)))
    assert np.all(got[ref[..., 0] == 1][:, 2] == 0.0)
    vmax = np.broadcast_to(np.nanmax(np.abs(ln.series_major(v, layout)), axis=1).astype(ln.LD)[None, :], got.shape[:2])
    dm = np.abs(got[..., 1].astype(ln.LD) - ref[..., 1])[~empty]
    bound_m = (ln.LD(1e-13) * vmax)[~empty]
    ok = ~np.isnan(ref[..., 2].astype(np.float64))
    ds = np.abs(got[..., 2].astype(ln.LD) - ref[..., 2])[ok]
    bound_s = (ln.LD(1e-12) * ref[..., 2] + ln.LD(1e-13) * vmax)[ok]
    worst = lambda d, bound: float((d[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0      # (a series of zeros: bound 0, met exactly)
    fig = {"mean_err_over_bound": worst(dm, bound_m), "std_err_over_bound": worst(ds, bound_s)}
    print(name, fig)
    record(name, fig)
    assert np.all(dm <= bound_m)
    assert np.all(ds <= bound_s)
    return fig


@pytest.mark.parametrize("name", MOMENT_CASES)
def test_moments(stats, name):
    v, lab, offset, order, ref, layout, s_nan = moment_case(name)
    got = stats.label_moments(v, offset, order, layout)
    check_moments(got, ref, v, "moments/" + name, layout)
    full = np.diff(offset).astype(np.float64)
    n = got[..., 0]
    others = [s for s in range(n.shape[1]) if s != s_nan and s != n.shape[1] - 1]
    assert all(np.array_equal(n[:, s], full) for s in others)       # the NaNs of one series reduce that series' n alone
    if full.max() > 1000:
        assert (n[:, s_nan] < full)[full > 1000].all()
    assert np.array_equal(stats.label_moments(v, offset, order, layout), got, equal_nan=True)      # two runs, the same bits


# ---- quantiles

QUANT_COUNTS = (1, 2, 3, SMALL_N - 1, SMALL_N, SMALL_N + 1, CHUNK - 1, CHUNK + 1, 65537, 0)


@functools.lru_cache(maxsize=None)
def quantile_case():
    rng = np.random.default_rng(21)
    lab = ln.scatter_labels(rng, 120000, list(QUANT_COUNTS))
    v = ln.pattern_series(rng, lab, len(QUANT_COUNTS))
    offset, order = ln.member_list(lab, len(QUANT_COUNTS))
    ref = ln.quantiles_numpy(v, offset, order, ln.Q_TEST)
    return frozen(lab, v, offset, order, ref)


def same_bits(a, b):
    """== in every entry (so -0.0 is 0.0), NaN where and only where the other has NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all((a == b) | np.isnan(a)))


def test_quantiles_equal_numpys(stats):
    lab, v, offset, order, ref = quantile_case()
    assert np.diff(offset).tolist() == list(QUANT_COUNTS)
    got = stats.label_quantiles(v, offset, order, ln.Q_TEST, "series")
    assert got.shape == (len(QUANT_COUNTS), len(ln.PATTERNS), len(ln.Q_TEST))
    for s, pat in enumerate(ln.PATTERNS):
        for l, n in enumerate(QUANT_COUNTS):
            assert same_bits(got[l, s], ref[l, s]), (pat, n, got[l, s], ref[l, s])
    assert np.isnan(got[-1]).all()                                  # the label without a member
    assert np.isnan(got[:-1, :10]).sum() == 0                       # every other (label, series) of the NaN-free patterns has its numbers
    # the adjacent-bucket patterns straddle the pair where the ranks allow it
    k = ln.PATTERNS.index("adj0")
    lo, hi = np.array(ln.ADJACENT[0], dtype=np.uint64).view(np.float64)
    big = QUANT_COUNTS.index(65537)
    assert lo < got[big, k, ln.Q_TEST.index(0.975)] < hi or got[big, k, ln.Q_TEST.index(0.975)] in (lo, hi)
    assert got[big, k, 0] == lo and got[big, k, -1] == hi
    # voxel-major: the same numbers read along the other axis
    assert same_bits(stats.label_quantiles(np.ascontiguousarray(v.T), offset, order, ln.Q_TEST, "voxel"), got)
    # two runs, the same bits; unsorted and repeated probabilities
    assert same_bits(stats.label_quantiles(v, offset, order, ln.Q_TEST, "series"), got)
    q2 = (0.75, 0.5, 0.5, 0.0)
    assert same_bits(stats.label_quantiles(v, offset, order, q2), got[:, :, [ln.Q_TEST.index(p) for p in q2]])


def test_quantiles_and_n_do_not_depend_on_the_voxel_order(stats):
    lab, v, offset, order, ref = quantile_case()
    base = stats.label_stats(v, lab, len(QUANT_COUNTS), ln.Q_TEST)
    perm = np.random.default_rng(22).permutation(lab.size)
    got = stats.label_stats(np.ascontiguousarray(v[:, perm]), lab[perm], len(QUANT_COUNTS), ln.Q_TEST)
    assert same_bits(got[..., 3:], base[..., 3:]) and np.array_equal(got[..., 0], base[..., 0])
    assert same_bits(base[..., 3:], ref)


def test_many_labels_above_and_below_small_n(stats):
    """257 labels, most of them below SMALL_N and the edge counts above: both paths of one call, with more series than a key tile of 8"""
    lab, offset, order, counts = index_case("L257")
    rng = np.random.default_rng(23)
    v = np.where(rng.random((9, lab.size)) < 0.4, 0.0, rng.standard_normal((9, lab.size)))
    got = stats.label_quantiles(v, offset, order, ln.Q_TEST)
    assert same_bits(got, ln.quantiles_numpy(v, offset, order, ln.Q_TEST))


# ---- the whole entry

def test_the_whole_entry_equals_the_stages(stats):
    v, lab, offset, order, ref, layout, s_nan = moment_case("L3_S60_voxel")
    L = len(offset) - 1
    got = stats.label_stats(v, lab, L, ln.Q_TEST, layout)
    assert got.shape == (L, 60, 3 + len(ln.Q_TEST))
    of, od = stats.label_index(lab, L)
    assert np.array_equal(got[..., :3], stats.label_moments(v, of, od, layout), equal_nan=True)
    assert same_bits(got[..., 3:], stats.label_quantiles(v, of, od, ln.Q_TEST, layout))
    assert same_bits(got[..., 3:], ln.quantiles_numpy(v, offset, order, ln.Q_TEST, layout))
    only = stats.label_stats(v, lab, L, (), layout)                 # no probability: the moments alone
    assert only.shape == (L, 60, 3) and np.array_equal(only, got[..., :3], equal_nan=True)
    dev = stats.label_stats(torch.as_tensor(v, device="cuda"), torch.as_tensor(lab, device="cuda"), L, ln.Q_TEST, layout)
    assert np.array_equal(dev, got, equal_nan=True)


def test_limits_and_return_codes(stats):
    lib = importlib.import_module(PKG + "._lib")
    Lb = lib.lib()
    assert stats.limits() == (stats.CHUNK, stats.SMALL_N, stats.MAX_LABEL, stats.MAX_SERIES, stats.MAX_Q)
    nvox = 64
    lab = torch.zeros(nvox, dtype=torch.int32, device="cuda")
    val = torch.ones(2 * nvox, dtype=torch.float64, device="cuda")
    out = torch.full((4096,), 7.0, dtype=torch.float64, device="cuda")
    off = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    ordr = torch.full((nvox,), 77, dtype=torch.int32, device="cuda")
    dq = lambda *q: (ctypes.c_double * len(q))(*q)
    ptr = lambda x: None if x is None else x.data_ptr()

    def whole(nv=nvox, label=lab, n_label=2, n_series=2, values=val, vs=1, ss=nvox, n_q=2, q=dq(0.25, 0.5), o=out):
        return Lb.met2_label_stats(0, nv, ptr(label), n_label, n_series, ptr(values), vs, ss, n_q, q, ptr(o), None)

    for bad in (1.5, -0.1, float("nan"), float("inf")):
        assert whole(q=dq(0.5, bad)) == E_INVALID
    assert whole(vs=0) == E_INVALID and whole(ss=0) == E_INVALID and whole(vs=-1) == E_INVALID and whole(ss=-3) == E_INVALID
    assert whole(label=None) == E_INVALID and whole(values=None) == E_INVALID and whole(o=None) == E_INVALID and whole(q=None) == E_INVALID
    assert whole(n_label=0) == E_INVALID and whole(n_series=0) == E_INVALID and whole(n_q=-1) == E_INVALID and whole(nv=-1) == E_INVALID
    assert whole(n_label=stats.MAX_LABEL + 1) == E_UNSUPPORTED and whole(n_series=stats.MAX_SERIES + 1) == E_UNSUPPORTED
    assert whole(n_q=stats.MAX_Q + 1, q=dq(*([0.5] * (stats.MAX_Q + 1)))) == E_UNSUPPORTED
    assert whole(nv=2 ** 31) == E_UNSUPPORTED                        # nothing is read
    # the stage entries
    idx = lambda nv=nvox, label=lab, n_label=2, offset=off, order=ordr: Lb.met2_label_index(0, nv, ptr(label), n_label, ptr(offset), ptr(order), None)
    assert idx(nv=-1) == E_INVALID and idx(n_label=0) == E_INVALID and idx(label=None) == E_INVALID and idx(offset=None) == E_INVALID
    assert idx(order=None) == E_INVALID and idx(n_label=stats.MAX_LABEL + 1) == E_UNSUPPORTED and idx(nv=2 ** 31) == E_UNSUPPORTED
    mom = lambda n_label=2, offset=off, order=ordr, n_series=2, values=val, vs=1, ss=nvox, o=out: Lb.met2_label_moments(
        0, n_label, ptr(offset), ptr(order), n_series, ptr(values), vs, ss, ptr(o), None)
    assert mom(offset=None) == E_INVALID and mom(order=None) == E_INVALID and mom(values=None) == E_INVALID and mom(o=None) == E_INVALID
    assert mom(vs=0) == E_INVALID and mom(ss=-1) == E_INVALID and mom(n_label=0) == E_INVALID and mom(n_series=0) == E_INVALID
    assert mom(n_label=stats.MAX_LABEL + 1) == E_UNSUPPORTED and mom(n_series=stats.MAX_SERIES + 1) == E_UNSUPPORTED
    qua = lambda n_label=2, offset=off, order=ordr, n_series=2, values=val, vs=1, ss=nvox, n_q=2, q=dq(0.25, 0.5), o=out: Lb.met2_label_quantiles(
        0, n_label, ptr(offset), ptr(order), n_series, ptr(values), vs, ss, n_q, q, ptr(o), None)
    assert qua(q=dq(0.5, 1.0000001)) == E_INVALID and qua(q=None) == E_INVALID and qua(n_q=0) == E_INVALID and qua(vs=0) == E_INVALID
    assert qua(offset=None) == E_INVALID and qua(order=None) == E_INVALID and qua(values=None) == E_INVALID and qua(o=None) == E_INVALID
    assert qua(n_q=stats.MAX_Q + 1, q=dq(*([0.5] * (stats.MAX_Q + 1)))) == E_UNSUPPORTED and qua(n_label=stats.MAX_LABEL + 1) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((off == 77).all()) and bool((ordr == 77).all())        # the checks came first: nothing was written
    # offsets that are no offsets are refused once they are read (off is still 77, 77, ...)
    assert mom() == E_INVALID and qua() == E_INVALID and bool((out == 7.0).all())
    # at the caps' edge the call runs: MAX_Q probabilities, and every voxel in label 0 of two
    q16 = tuple(np.linspace(0.0, 1.0, stats.MAX_Q))
    assert whole(n_q=stats.MAX_Q, q=dq(*q16)) == 0
    got = out[:2 * 2 * (3 + stats.MAX_Q)].cpu().numpy().reshape(2, 2, -1)
    assert got[0, :, 0].tolist() == [64.0, 64.0] and np.all(got[0, :, 1] == 1.0) and np.all(got[0, :, 2] == 0.0) and np.all(got[0, :, 3:] == 1.0)
    assert got[1, :, 0].tolist() == [0.0, 0.0] and np.isnan(got[1, :, 1:]).all()
    with pytest.raises(ValueError):
        stats.label_stats(np.ones((2, 8)), np.zeros(9, dtype=np.int32), 2)
    with pytest.raises(ValueError):
        stats.label_stats(np.ones((2, 8)), np.zeros(8), 2)           # labels must be integers
    with pytest.raises(ValueError):
        stats.label_stats(np.ones((2, 8)), np.zeros(8, dtype=np.int32), 2, layout="rows")
    with pytest.raises(lib.Met2Error):
        stats.label_stats(np.ones((2, 8)), np.zeros(8, dtype=np.int32), 2, q=(0.5, 2.0))


# ---- the drivers

def driver_volume():
    """16 x 16 x 8 x 32: a two-pool decay whose amplitude follows a smooth field, three tissue levels, 1 % noise; the mask leaves a rim out
    (the volume of tests/test_gpu_seg.py and tests/test_gpu_pve.py)"""
    rng = np.random.default_rng(20261019)
    nx, ny, nz, nt = 16, 16, 8, 32
    TE = 10.0 * np.arange(1, nt + 1)
    x, y, z = np.meshgrid(np.linspace(-1, 1, nx), np.linspace(-1, 1, ny), np.linspace(-1, 1, nz), indexing="ij")
    rr = x * x + y * y
    amp = np.where(rr < 0.15, 500.0, np.where(rr < 0.5, 800.0, 1100.0)) * np.exp(0.2 * x - 0.1 * y + 0.1 * z)
    sig = amp[..., None] * (0.15 * np.exp(-TE / 20.0) + 0.85 * np.exp(-TE / 80.0))
    data = sig * (1.0 + 0.01 * rng.standard_normal(sig.shape))
    mask = ((np.abs(x) < 0.9) & (np.abs(y) < 0.9)).astype(np.int64)
    return data, mask, TE


def restated(motor, res, labels, q):
    """the dict of label_stats_filter by the restatement, from the run's own arrays: labels > 0 to dense indices, the eight maps, the spectra"""
    ids = np.unique(labels)
    ids = ids[ids > 0]
    dense = np.full(labels.shape, -1, dtype=np.int32)
    for i, x in enumerate(ids):
        dense[labels == x] = i
    offset, order = ln.member_list(dense, ids.size)
    maps = np.stack([np.asarray(res[k], dtype=np.float64).reshape(-1) for k in motor.STAT_QUANTITIES])
    fsol = np.asarray(res["fsol_4D"], dtype=np.float64).reshape(-1, res["fsol_4D"].shape[-1])
    mo, sm = ln.moments(maps, offset, order), ln.moments(fsol, offset, order, "voxel")
    tot = sm[..., 1].astype(np.float64).sum(axis=1)
    return {"labels": ids, "moments": mo, "tot": tot, "quantiles": ln.quantiles_numpy(maps, offset, order, q), "maps": maps,
            "spectrum_mean": sm[..., 1] / tot[:, None], "spectrum_quantiles": ln.quantiles_numpy(fsol, offset, order, q, "voxel") / tot[:, None, None], "fsol": fsol}


def check_against_restatement(got, want, name):
    """got: n, mean, std, quantiles, spectrum_mean, spectrum_quantiles of L labels"""
    st = np.concatenate([got["n"][..., None], got["mean"][..., None], got["std"][..., None]], axis=-1)
    check_moments(st, want["moments"], want["maps"], name)
    assert same_bits(got["quantiles"], want["quantiles"])
    # a bin's mean is within 1e-13 max|bin| of the restatement's (the header's bound); the normalising sum of the 60 means then within
    # rel = sum_b 1e-13 max|bin b| / sum + 64 * 2^-53 (its own additions), and the quotient rounds once more
    vmax = np.abs(want["fsol"]).max(axis=0)
    tot = want["tot"]
    rel = 1e-13 * vmax.sum() / tot + 66 * 2.0 ** -53
    ref = want["spectrum_mean"].astype(np.float64)
    assert np.all(np.abs(got["spectrum_mean"] - ref) <= 1e-13 * vmax[None, :] / tot[:, None] + rel[:, None] * ref)
    assert np.all(np.abs(got["spectrum_mean"].sum(axis=-1) - 1.0) <= 64 * 2.0 ** -53)
    # the band is the exact quantile over the device's own sum
    refq = want["spectrum_quantiles"]
    assert np.array_equal(np.isnan(got["spectrum_quantiles"]), np.isnan(refq))
    assert np.all(np.abs(got["spectrum_quantiles"] - refq) <= rel[:, None, None] * np.abs(refq))


def test_drivers_take_tissue_stats(motor, stats, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    plan_mod = importlib.import_module(PKG + ".plan")
    data, mask, TE = driver_volume()
    args = (mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    vox = (2.0, 2.5, 4.0)
    thr = 0.9
    off = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="pve", return_prepared=True)
    on = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="pve", tissue_stats="yes", pve_threshold=thr,
                                 return_prepared=True)
    assert sorted(on) == sorted(list(off) + ["tissue_stats"])
    for k in off:                                                    # the ten outputs and the segmentation: what they were
        assert np.array_equal(on[k], off[k], equal_nan=True), k
    ts = on["tissue_stats"]
    # the labels of THIS run's own partial-volume maps
    lab = np.zeros(mask.shape, dtype=np.int32)
    for k in range(3):
        lab[on["TWC_pve"][k] > thr] = k + 1
    assert np.array_equal(lab, motor.tissue_labels(on, "pve", thr)) and lab.any()
    whole = (on["TWC_seg"] > 0).astype(np.int32)
    q = stats.DEFAULT_Q
    want = restated(motor, on, lab, q)
    assert np.array_equal(ts["labels"], want["labels"]) and ts["quantities"] == motor.STAT_QUANTITIES and np.array_equal(ts["q"], q)
    assert np.array_equal(ts["T2s"], on["T2s"])
    check_against_restatement(ts, want, "driver/tissues")
    want_all = restated(motor, on, whole, q)
    check_against_restatement({k: ts["all"][k][None] for k in motor.STAT_KEYS}, want_all, "driver/all")
    assert ts["all"]["n"][0] == whole.sum()
    # the fit of the mean signals: recon_met2_rois by hand on the same labels, the prepared data and the run's flip angles
    L = want["labels"].size
    plan = plan_mod.Met2Plan(32, 60, 91, device=0, myelin_T2=40.0)
    try:
        T2s = on["T2s"]
        plan.build_dictionary_epg(T2s, 1000.0 * np.ones_like(T2s), float(TE[1] - TE[0]), np.linspace(90.0, 180.0, 91), 3000.0)
        Id = motor.create_Laplacian_matrix(60, 0)
        hand = [motor.recon_met2_rois(on["data_prepared"], r, on["FA_index"], None, T2s, Id, factor=1.01, myelin_T2=40.0, plan=plan) for r in (lab, whole)]
        assert ts["mean_signal_fsol"].shape == (L + 1, 60)
        assert np.array_equal(ts["mean_signal_fsol"], np.concatenate([h["fsol"] for h in hand]))
        for name in ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC"):
            assert np.array_equal(ts["mean_signal_" + name], np.concatenate([h[name] for h in hand])), name
        # a caller's own plan: the volume on the device in one piece, the same numbers
        plan.set_penalty("L2", T2s)
        own = motor.recon_met2_arrays(data, *args, plan=plan, bias_correct="yes", voxel_size=vox, segment="pve", tissue_stats="yes", pve_threshold=thr)
    finally:
        plan.close()
    for k in ("n", "mean", "std", "quantiles", "spectrum_mean", "spectrum_quantiles", "mean_signal_fsol"):
        assert np.array_equal(own["tissue_stats"][k], ts[k], equal_nan=True), k
    # segment='yes': the hard labels
    hard = motor.label_stats_filter(on, on["TWC_seg"].astype(np.int32))
    assert hard["labels"].tolist() == [1, 2, 3]
    check_against_restatement(hard, restated(motor, on, on["TWC_seg"].astype(np.int32), q), "driver/hard")
    assert np.array_equal(hard["n"][:, 0], np.bincount(on["TWC_seg"].reshape(-1), minlength=4)[1:])
    with pytest.raises(ValueError, match="integer"):
        motor.label_stats_filter(on, on["TWC"])
    with pytest.raises(ValueError, match="no label"):
        motor.label_stats_filter(on, np.zeros(mask.shape, dtype=np.int32))
    # the on-disk driver: the two tables read back to the dict
    aff = np.diag([2.0, -2.5, 4.0, 1.0])
    nifti.save(nifti.NiftiImage(data, aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(mask.astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/ts_"
    disk = motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force", "no",
                                  40.0, bias_correct="yes", segment="pve", tissue_stats="yes")
    dts = disk["tissue_stats"]
    for k in ("n", "mean", "std", "quantiles", "spectrum_mean"):     # (not the mean signals: they are summed in memory order, and this volume is Fortran-ordered)
        assert np.array_equal(dts[k], ts[k], equal_nan=True), k
    rows = [line.split(",") for line in open(out + "table_tissue_stats.csv").read().split()]
    assert len(rows) == 8 * (L + 1) and all(len(r) == 5 + len(q) for r in rows)
    assert [r[0] for r in rows[::8]] == [str(int(x)) for x in dts["labels"]] + ["all"] and [r[1] for r in rows[:8]] == list(motor.STAT_QUANTITIES)
    num = np.array([[float(x) for x in r[2:]] for r in rows]).reshape(L + 1, 8, -1)
    assert np.array_equal(num[:L, :, 0], dts["n"]) and np.array_equal(num[:L, :, 1], dts["mean"], equal_nan=True)
    assert np.array_equal(num[:L, :, 2], dts["std"], equal_nan=True) and np.array_equal(num[:L, :, 3:], dts["quantiles"], equal_nan=True)
    assert np.array_equal(num[L, :, 1], dts["all"]["mean"], equal_nan=True)
    spec = np.loadtxt(out + "table_tissue_spectra.csv", delimiter=",")
    assert spec.shape == (1 + 2 * (L + 1), 60) and np.array_equal(spec[0], dts["T2s"])
    assert np.array_equal(spec[1::2], np.vstack([dts["spectrum_mean"], dts["all"]["spectrum_mean"]])) and np.array_equal(spec[2::2], dts["mean_signal_fsol"])
    with pytest.raises(ValueError, match="needs segment"):
        motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force",
                               "no", 40.0, tissue_stats="yes")
