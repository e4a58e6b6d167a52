"""numpy restatement of the label statistics (met2_label_index / _moments / _quantiles / _stats in include/met2_hip.h): the member list by a
stable argsort, mean and std in long double, quantiles by np.sort and the order-statistic formula of the header.  `values` is [S, nvox]
(layout 'series') or [nvox, S] ('voxel'); `labels` [nvox] integers, members are 0 .. n_label-1."""
import numpy as np

LD = np.longdouble
CHUNK = 16384
SMALL_N = 1024
Q_TEST = (0.0, 0.025, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.975, 1.0)


def member_list(labels, n_label):
    """-> (offset [n_label + 1] int32, order [members] int32): by ascending label, inside a label by ascending voxel index"""
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    idx = np.nonzero((lab >= 0) & (lab < n_label))[0]
    order = idx[np.argsort(lab[idx], kind="stable")]
    offset = np.concatenate(([0], np.cumsum(np.bincount(lab[idx], minlength=n_label))))
    return offset.astype(np.int32), order.astype(np.int32)


def series_major(values, layout):
    v = np.asarray(values, dtype=np.float64)
    return v.reshape(v.shape[0], -1) if layout == "series" else v.reshape(-1, v.shape[-1]).T


def samples(values, offset, order, layout="series"):
    """yields (label, series, sample): the members' values that are not NaN, -0.0 as +0.0, in member order"""
    v = series_major(values, layout)
    for l in range(len(offset) - 1):
        mem = order[offset[l]:offset[l + 1]]
        for s in range(v.shape[0]):
            x = v[s, mem]
            yield l, s, x[~np.isnan(x)] + 0.0


def moments(values, offset, order, layout="series"):
    """-> [L, S, 3] long double: n, mean, std (ddof 1, two passes; 0 for n = 1; NaN without a value)"""
    S = series_major(values, layout).shape[0]
    out = np.full((len(offset) - 1, S, 3), np.nan, dtype=LD)
    for l, s, x in samples(values, offset, order, layout):
        n = x.size
        out[l, s, 0] = n
        if n:
            xl = x.astype(LD)
            mean = xl.sum() / LD(n)
            out[l, s, 1] = mean
            out[l, s, 2] = np.sqrt(((xl - mean) ** 2).sum() / LD(n - 1)) if n > 1 else LD(0)
    return out


def quantile_sorted(s, q):
    """the header's formula on a sorted sample: h = (n - 1) q, the order statistics floor(h) and floor(h) + 1, numpy's _lerp"""
    n = s.size
    h = np.float64(n - 1) * np.float64(q)
    fl = np.floor(h)
    i0 = int(fl)
    i1 = i0 + 1
    if h >= n - 1:
        i0 = i1 = n - 1
    g = h - fl
    a, b = s[i0], s[i1]
    d = b - a
    return b - d * (np.float64(1.0) - g) if g >= 0.5 else a + d * g


def quantiles(values, offset, order, q, layout="series"):
    """-> [L, S, n_q] by np.sort and quantile_sorted; NaN without a value"""
    S = series_major(values, layout).shape[0]
    out = np.full((len(offset) - 1, S, len(q)), np.nan)
    for l, s, x in samples(values, offset, order, layout):
        if x.size:
            xs = np.sort(x)
            out[l, s] = [quantile_sorted(xs, p) for p in q]
    return out


def quantiles_numpy(values, offset, order, q, layout="series"):
    """the same by np.quantile(sample, q, method='linear') of the installed numpy"""
    S = series_major(values, layout).shape[0]
    out = np.full((len(offset) - 1, S, len(q)), np.nan)
    for l, s, x in samples(values, offset, order, layout):
        if x.size:
            out[l, s] = np.quantile(x, np.asarray(q, dtype=np.float64), method="linear")
    return out


def scatter_labels(rng, nvox, counts, n_label=None):
    """labels [nvox] with counts[l] members of label l scattered at random; the rest of the voxels get -1 or n_label (non-members) in turn"""
    n_label = len(counts) if n_label is None else n_label
    total = int(np.sum(counts))
    assert total <= nvox
    lab = np.where(np.arange(nvox) % 2 == 0, -1, n_label).astype(np.int32)
    pos = rng.permutation(nvox)[:total]
    lab[pos] = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    return lab


# the two order statistics of a quantile in adjacent buckets: ...FF / ...00 carried across 7, 6, 4 and 1 bytes of the key
ADJACENT = ((0x3FFFFFFFFFFFFFFF, 0x4000000000000000), (0x3FF0FFFFFFFFFFFF, 0x3FF1000000000000), (0x3FF00000FFFFFFFF, 0x3FF0000100000000),
            (0x3FF00000000000FF, 0x3FF0000000000100))
PATTERNS = ("gauss", "equal", "two", "zeros40", "signs", "lastbyte", "adj0", "adj1", "adj2", "adj3", "nan10")


def pattern_series(rng, labels, n_label):
    """[len(PATTERNS), nvox]: the value patterns of the quantile tests, one series each"""
    nvox = labels.size
    v = np.empty((len(PATTERNS), nvox))
    v[0] = rng.standard_normal(nvox)
    v[1] = 3.25
    v[2] = rng.choice([1.5, -2.25], nvox)
    v[3] = np.where(rng.random(nvox) < 0.4, 0.0, 0.1 * np.abs(rng.standard_normal(nvox)))        # the MWF's pattern
    pool = np.array([-0.0, 0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1.0, -1.0, 0.5, -0.5])
    v[4] = np.where(rng.random(nvox) < 0.7, rng.choice(pool, nvox), rng.standard_normal(nvox))
    v[5] = 1.0 + rng.integers(0, 256, nvox) * 2.0 ** -52
    offset, order = member_list(labels, n_label)
    for k, (a, b) in enumerate(ADJACENT):
        lo, hi = np.array([a, b], dtype=np.uint64).view(np.float64)
        row = np.full(nvox, hi)
        for l in range(n_label):
            mem = order[offset[l]:offset[l + 1]]
            cut = int(np.floor((mem.size - 1) * 0.975)) + 1 if mem.size else 0       # ranks floor(h) and floor(h) + 1 of q = 0.975 straddle the pair
            row[rng.permutation(mem)[:cut]] = lo
        v[6 + k] = row
    v[10] = np.where(rng.random(nvox) < 0.1, np.nan, rng.standard_normal(nvox))
    return v
