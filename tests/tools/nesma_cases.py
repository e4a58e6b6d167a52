"""Inputs and numpy references for the tests of nesma_kernel (tests/test_gpu_prefilters.py): which of met2_nesma's six launches an echo
count takes, the two-class volumes whose pairs lie near the 2.5 % threshold, the integer volumes whose pairs lie ON it, and the filter
itself (motor:305-333) written once more with numpy, for the shares, the ties and the exact integer reference."""
import functools
import warnings

import numpy as np

HW = 6                                          # the window is [x-6, x+6) x [y-6, y+6) x [z-6, z+6), clipped
THRESHOLD = 2.5                                 # per cent

# met2_nesma's dispatch on the echo count, first match wins: (instantiation <NE, PACK, NT>, condition)
DISPATCH = (
    ("one echo", lambda nt: nt == 1),           # nesma_one_echo_kernel; the others are nesma_kernel<NE, PACK, NT>
    ("<1,2,32>", lambda nt: nt == 32),
    ("<1,2,0>", lambda nt: nt < 32),
    ("<1,1,48>", lambda nt: nt == 48),
    ("<1,1,0>", lambda nt: nt <= 64),
    ("<2,1,0>", lambda nt: nt <= 128),
)


def launch(nt):
    assert 1 <= nt <= 128
    return next(name for name, cond in DISPATCH if cond(nt))


def sum_branch(nt):
    """the path of np_rowsum_group (numpy's pairwise sum below its block size of 128)"""
    if nt < 8:
        return "in order"
    return "8 sums" if nt % 8 == 0 else "8 sums + tail of %d" % (nt % 8)


NT_A = (1, 7, 8, 9, 16, 31, 32, 33, 40, 63, 64, 48, 65, 72, 127, 128)
BIG = (6, 7, 13)
CASES_A = ([(BIG, nt) for nt in NT_A]
           + [((3, 4, nz), nt) for nz in (1, 2, 3, 5, 9) for nt in (9, 32, 40, 72)]
           + [((14, 1, 1), 16), ((1, 14, 1), 16), ((3, 4, 5), 48), ((3, 4, 5), 1)])
NT_TIES = (2, 8, 9, 31, 32, 33, 48, 63, 64, 65, 127, 128)
SHAPE_TIES = (4, 5, 13)
SD = 0.022
SEEDS = {}                                      # (shape, nt) -> seed, where the default seed misses the CPU conditions


def z_runs(shape):
    """the lengths of the window's z-run (the kernel's L) that occur in a volume"""
    nz = shape[2]
    return sorted({min(z + HW, nz) - max(z - HW, 0) for z in range(nz)})


def window(shape, x, y, z):
    return tuple(slice(max(c - HW, 0), min(c + HW, n)) for c, n in zip((x, y, z), shape))


@functools.lru_cache(maxsize=None)
def case_a(shape, nt, forced=()):
    """-> (data [nx,ny,nz,nt] already multiplied by the mask, mask int64, the mask-3 voxel, the all-zero voxel).  Two decay classes with
    2.2 % noise, about a fifth of the voxels masked out; `forced`: voxels that stay in the mask.  The arrays are shared: do not write."""
    nx, ny, nz = shape
    rng = np.random.default_rng(SEEDS.get((shape, nt), 1000 * nt + nx * ny * nz))
    base = rng.uniform(0.5, 2.0, size=(2, nt)) * np.exp(-np.arange(nt) / 12.0)
    lab = rng.integers(0, 2, size=shape)
    d = base[lab] * (1.0 + SD * rng.standard_normal(shape + (nt,)))
    m = (rng.uniform(size=shape) > 0.2).astype(np.int64)
    three = np.unravel_index(1, shape)
    zero = np.unravel_index(nx * ny * nz - 1, shape)
    for v in forced:
        m[v] = 1
    m[three] = 3                                                    # only mask == 1 is filtered
    m[zero] = 1; d[zero] = 0.0                                      # sum 0: similar to nothing, a NaN row
    d = d * m[..., None]
    d.setflags(write=False); m.setflags(write=False)
    return d, m, three, zero


ONE_ECHO_SHAPE = (12, 12, 13)


@functools.lru_cache(maxsize=None)
def one_echo_case():
    """one echo, one class, 0.4 % noise on [12,12,13]: every neighbour is similar, so the voxels in the middle take the mean of all 12^3,
    the longest vector the one-echo kernel sums; towards the corners every count from 6^3 on"""
    d = 1.0 + 0.004 * np.random.default_rng(11).standard_normal(ONE_ECHO_SHAPE + (1,))
    m = np.ones(ONE_ECHO_SHAPE, dtype=np.int64)
    m[3, 4, 5] = 0; d[3, 4, 5] = 0.0
    d.setflags(write=False); m.setflags(write=False)
    return d, m


def relative_distances(d, m):
    """RE [%] of every (centre, neighbour) pair of the windows of the centres with mask == 1, as one vector"""
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for x, y, z in zip(*np.nonzero(m == 1)):
            c = d[x, y, z]
            rows = d[window(m.shape, x, y, z)].reshape(-1, d.shape[-1])
            out.append(100 * np.sum(np.abs(rows - c), axis=1) / np.sum(c))
    return np.concatenate(out)


def shares(d, m):
    """(share of the pairs with |RE - 2.5| < 0.25, share of the similar pairs, number of pairs)"""
    re = relative_distances(d, m)
    return float(np.mean(np.abs(re - THRESHOLD) < 0.1 * THRESHOLD)), float(np.mean(re < THRESHOLD)), re.size


def nesma_numpy(d, m):
    """the filter in numpy's own floating point: np.sum over the echoes, np.mean over the similar rows"""
    out = np.zeros_like(d, dtype=np.float64)
    nt = d.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)             # np.mean of no row: nan, as in the reference
        for x, y, z in zip(*np.nonzero(m == 1)):
            c = d[x, y, z]
            rows = d[window(m.shape, x, y, z)].reshape(-1, nt)
            re = 100 * np.sum(np.abs(rows - c), axis=1) / np.sum(c)
            out[x, y, z] = np.mean(rows[re < THRESHOLD, :], axis=0)
    return out


def window_mean(d):
    """every voxel the mean of its whole window, rows added in the window's order"""
    out = np.empty_like(d)
    for x, y, z in np.ndindex(*d.shape[:3]):
        out[x, y, z] = np.mean(d[window(d.shape[:3], x, y, z)].reshape(-1, d.shape[-1]), axis=0)
    return out


# ------------------------------------------------------------------ integer volumes: pairs ON the threshold
def tie_vectors(nt):
    """(base, u): integers with sum(base) = 8000, sum(u) = 0, sum|u| = 50, u non-zero on as many echoes as nt allows (first and last among
    them), signs alternating"""
    w = np.exp(-np.arange(nt) / 12.0)
    base = np.floor(8000 * w / w.sum()).astype(np.int64)
    base[0] += 8000 - base.sum()
    k = min(nt, 50)
    pos = np.round(np.linspace(0, nt - 1, k)).astype(np.int64)
    u = np.zeros(nt, dtype=np.int64)
    for sign, idx in ((1, pos[0::2]), (-1, pos[1::2])):
        share = np.full(idx.size, 25 // idx.size, dtype=np.int64)
        share[:25 % idx.size] += 1
        u[idx] = sign * share
    return base, u


@functools.lru_cache(maxsize=None)
def tie_case(nt):
    """integer volume [4,5,13,nt] (int64): row(v) = base + a(v) u with a in 0..8, so that for every pair S = 50 |a - a'| and sumc = 8000:
    RE is exactly 2.5 at |a - a'| = 4"""
    base, u = tie_vectors(nt)
    a = np.random.default_rng(77 + nt).integers(0, 9, size=SHAPE_TIES)
    d = base + a[..., None] * u
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def tie_reference(nt):
    """-> (filtered volume, number of pairs with RE == 2.5 exactly, number of pairs) in int64 arithmetic: similar iff 40 S < sumc; the row
    is the integer sum of the similar rows, divided once by their count"""
    d = tie_case(nt)
    out = np.empty(d.shape, dtype=np.float64)
    ties = pairs = 0
    for x, y, z in np.ndindex(*SHAPE_TIES):
        c = d[x, y, z]
        rows = d[window(SHAPE_TIES, x, y, z)].reshape(-1, nt)
        S = np.abs(rows - c).sum(axis=1)
        sumc = int(c.sum())
        sim = 40 * S < sumc
        ties += int(np.sum(40 * S == sumc)); pairs += S.size
        out[x, y, z] = rows[sim].sum(axis=0).astype(np.float64) / float(sim.sum())
    out.setflags(write=False)
    return out, ties, pairs


# ------------------------------------------------------------------ signs and non-finite values
def negative_case():
    """every echo negative: sumc < 0, RE <= 0 for every neighbour, all are similar"""
    return -np.abs(np.random.default_rng(5).standard_normal((3, 4, 5, 9))) - 0.01


def zero_sum_case():
    """echoes k (+1, -1, 0, ...), k = 1..3: sumc == 0 with non-zero echoes; S / 0 is inf or nan, never similar"""
    k = np.random.default_rng(6).integers(1, 4, size=(2, 2, 3))
    row = np.zeros(8); row[0] = 1.0; row[1] = -1.0
    return k[..., None] * row


NONFINITE = {(1, 2, 5): np.nan, (2, 1, 8): np.inf, (2, 3, 3): -np.inf}     # interior voxels of the 4x5x13 volume, one echo each


def nonfinite_case():
    d, m, three, zero = case_a(SHAPE_TIES, 32, forced=tuple(NONFINITE))
    d = d.copy()
    for i, (v, val) in enumerate(NONFINITE.items()):
        d[v][3 + 11 * i] = val
    return d, m
