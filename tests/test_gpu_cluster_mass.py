"""The cluster mass on the device (MET2_TFCE_MODE_MASS; include/met2_hip.h states the definition) against its numpy restatement
(tests/tools/cluster_mass_numpy.py: scipy.ndimage.label and an int64 np.add.at, independent of union-find and of atomics).
Equality.  A member contributes an integer, the integers are summed in 64 bits (no order dependence) and the total is converted once,
round to nearest even, then scaled by a power of two: out, kmax, first and count must EQUAL the restatement bit for bit, at connectivity
6, 18 and 26, with and without a mask, on every case of CASES -- the smallest shapes at which the kernels can go wrong (wave and block ends,
rows that end next to each other in memory, one root fed by every wave and block, many roots per wave, the threshold, ties, saturation, values
that are not numbers, nothing above the threshold).  Before any device call a case asserts on the restatement that it has the structure it is
named for.  The same from the device alone: a map's bits do not depend on K, its place, its batch mates or on mirroring.
Group entries (t, F, the pseudo-t): first, kmax and count equal group.cluster_mass of the statistic maps the plain entries return, and the
restatement; count accumulates over launches; refusals come before device work and change no output.
End to end: randomise, group_stats_filter and motor_group_stats on the device equal the host run with the stand-ins, key for key.
With MET2_GROUP_MASS_PARITY_OUT=<file> the module writes what it compared and measured there (profiles/group_mass_parity.json)."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cluster_mass_numpy as cm                                    # noqa: E402
import group_f_numpy as gf                                         # noqa: E402
import group_numpy as gn                                           # noqa: E402
import group_vsm_numpy as gv                                       # noqa: E402
import tfce_numpy as tn                                            # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
INVALID, UNSUPPORTED = -1, -2
MAX_K = 32
CONN = (6, 18, 26)
U = 2.0 ** -24
MEASURED = {"maps_compared": 0, "cells_compared": 0, "cells_that_differ": 0, "group_values_compared": 0, "group_values_that_differ": 0,
            "worst_error_over_e_2^-25": 0.0}


@pytest.fixture(scope="module")
def group():
    g = importlib.import_module(PKG + ".group")
    assert g.MODES["mass"] == 3 and g.tfce_limits()["max_k"] == MAX_K
    yield g
    path = os.environ.get("MET2_GROUP_MASS_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"measured": MEASURED, "reference": "tests/tools/cluster_mass_numpy.py (scipy.ndimage.label, int64 np.add.at)",
                       "measure": "float64 bit patterns of out, kmax, first and count that differ from the reference; the worst |out - long double "
                                  "sum of the raw statistic| / (e 2^-25) over the members of the planted case's observed and permuted t maps",
                       "bound": "0 differing values; the ratio stays below 1 + one rounding of the result", "device": torch.cuda.get_device_name(0)},
                      f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib").lib()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    return np.shape(got) == np.shape(want) and np.array_equal(bits(got), bits(want))


def tally(got, want, group_entry=False):
    a, b = ("group_values_compared", "group_values_that_differ") if group_entry else ("cells_compared", "cells_that_differ")
    MEASURED[a] += int(np.size(want))
    MEASURED[b] += int((bits(got) != bits(want)).sum()) if np.shape(got) == np.shape(want) else int(np.size(want))


# ---------------------------------------------------------------- the cases: name -> (t [nx, ny, nz], h, mask or None)

def ncomp(t, h, conn, mask=None):
    return int(ndimage.label(cm.members(t, h, mask), structure=tn.structure(conn))[1])


def values(shape, seed, lo=1.0, hi=4.0):
    """values with bits below 2^-24, so that the quantisation rounds"""
    return np.random.default_rng(seed).uniform(lo, hi, shape)


def random_mask(shape, seed):
    return (np.random.default_rng(seed).random(shape) < 0.8).astype(np.uint8)


def line(n, seed):
    """along z: a long run that crosses every wave and block end, broken by a few sub-threshold voxels"""
    t = values((1, 1, n), seed)
    t[0, 0, ::23] = 0.25
    return t, 1.0, random_mask((1, 1, n), seed + 1) if n > 2 else None


def full_line(n, seed):
    """one component of n voxels along z: its root, voxel 0, is fed from every wave of every block"""
    t = values((1, 1, n), seed)
    assert ncomp(t, 1.0, 6) == 1
    return t, 1.0, None


def row_ends(shape):
    """voxels that follow each other in memory across the end of a row (z) and of a plane (y): none are neighbours under 6"""
    nx, ny, nz = shape
    t = np.zeros(shape)
    v = values(shape, 77, 2.0, 3.0)
    for x in range(0, nx - 1, 4):
        for idx in ((x, 0, nz - 1), (x, 1, 0), (x, ny - 1, nz - 1), (x + 1, 0, 0)):
            t[idx] = v[idx]
    lit = int((t > 0).sum())
    assert ncomp(t, 1.0, 6) == lit and ncomp(t, 1.0, 26) < lit
    return t, 1.0, None


def full_block():
    """all of 16 x 16 x 4 above the threshold (the serpentine of tests/test_gpu_tfce.py with every voxel lit): ONE component whose root, voxel 0,
    is fed by every wave of all four blocks"""
    t = values((16, 16, 4), 51)
    assert ncomp(t, 1.0, 6) == 1 and t.size == 4 * 256
    return t, 1.0, None


def snake():
    """a 6-connected path between walls on 16 x 16 x 4: in the layers z = 0 and z = 2 the rows of even x are lit and joined at alternating ends,
    and one voxel at z = 1 joins the two layers: one component under 6 whose parent chains are long; without the joint there are two"""
    t = np.full((16, 16, 4), 0.5)
    v = values(t.shape, 58)
    for z in (0, 2):
        t[0::2, :, z] = v[0::2, :, z]
        for x in range(1, 15, 2):
            y = 15 if x % 4 == 1 else 0
            t[x, y, z] = v[x, y, z]
    t[0, 0, 1] = v[0, 0, 1]
    cut = t.copy()
    cut[0, 0, 1] = 0.5
    assert ncomp(t, 1.0, 6) == 1 and ncomp(cut, 1.0, 6) == 2 and int((t >= 1.0).sum()) == 2 * (8 * 16 + 7) + 1
    return t, 1.0, None


def checkerboard():
    x, y, z = np.indices((8, 8, 8))
    t = np.where((x + y + z) % 2 == 0, values((8, 8, 8), 52), 0.0)
    lit = int((t > 0).sum())
    assert ncomp(t, 1.0, 6) == lit and ncomp(t, 1.0, 18) == 1 and ncomp(t, 1.0, 26) == 1
    return t, 1.0, None


def pairs():
    """under 6, 128 components of two voxels, (x, y, 0) the root and (x, y, 1) its child: a wave adds to 16 distinct roots"""
    x, y, z = np.indices((16, 16, 2))
    t = np.where((x + y) % 2 == 0, values((16, 16, 2), 53), 0.0)
    assert ncomp(t, 1.0, 6) == 128 and ncomp(t, 1.0, 18) == 1
    return t, 1.0, None


def wall():
    t = values((9, 5, 3), 54)
    mask = np.ones((9, 5, 3), dtype=np.uint8)
    mask[4] = 0
    for conn in CONN:
        assert ncomp(t, 1.0, conn, mask) == 2 and ncomp(t, 1.0, conn) == 1
    return t, 1.0, mask


def edge_values():
    """the threshold and one ulp below it, ties at q + 1/2 towards an even and an odd q, the cap, above it, +infinity, and what joins nothing"""
    h = 3 * 0.3
    t = values((6, 5, 4), 55, 0.2, 2.0)
    t[0, 0, 0], t[0, 0, 1] = h, np.nextafter(h, 0)
    t[1, 1, 1], t[1, 1, 2] = (2.0 ** 24 + 0.5) * U, (2.0 ** 24 + 1.5) * U
    t[2, 2, 2], t[2, 2, 3], t[2, 3, 3] = cm.T_CAP, cm.T_CAP * 4, np.inf
    t[3, 0, 0], t[3, 1, 1], t[3, 2, 2], t[3, 3, 3] = np.nan, -np.inf, -0.0, np.nan
    t[5, 4, 3] = np.nextafter(cm.T_CAP, 0)
    mem = cm.members(t, h)
    assert mem[0, 0, 0] and not mem[0, 0, 1] and not mem[3].reshape(-1)[[0, 5, 10, 15]].any()
    assert cm.quantise(t[1, 1, 1]) == 2 ** 24 and cm.quantise(t[1, 1, 2]) == 2 ** 24 + 2 and cm.transform(t, h).max() >= 3 * cm.T_CAP
    return t, h, random_mask(t.shape, 56)


def nothing_above():
    t = values((5, 4, 3), 57, -1.0, 0.9)
    t[0, 0, 0] = np.nan
    assert not cm.members(t, 1.0).any()
    return t, 1.0, None


def smooth(shape, seed):
    t = ndimage.uniform_filter(np.random.default_rng(seed).standard_normal(shape), 3, mode="constant") * 3.0
    return t, float(t.max()) / 3.0, random_mask(shape, seed + 1)


CASES = {"1x1x1": lambda: (np.full((1, 1, 1), 3.2), 2.0, None), "1x1x1_below": lambda: (np.full((1, 1, 1), 1.2), 2.0, None)}
for _n in (63, 64, 65, 256, 257):
    CASES["line_z_%d" % _n] = lambda n=_n: line(n, n)
    CASES["full_line_z_%d" % _n] = lambda n=_n: full_line(n, n + 900)
CASES.update({
    "row_ends_65x3x2": lambda: row_ends((65, 3, 2)), "row_ends_3x65x2": lambda: row_ends((3, 65, 2)),
    "random_65x3x2": lambda: smooth((65, 3, 2), 41), "random_3x65x2": lambda: smooth((3, 65, 2), 43),
    "serpentine_all_of_16x16x4": full_block, "snake_between_walls": snake,
    "checkerboard": checkerboard, "pairs_16_roots_per_wave": pairs, "wall_of_mask_zeros": wall,
    "threshold_tie_cap_nan": edge_values, "nothing_above_the_threshold": nothing_above, "smooth_33x17x9": lambda: smooth((33, 17, 9), 45),
})


@pytest.mark.parametrize("name", sorted(CASES))
def test_out_and_kmax_equal_the_restatement(group, name):
    t, h, mask = CASES[name]()
    for m in ((None,) if mask is None else (None, mask)):
        for conn in CONN:
            want, want_max = cm.spatial(t[None], m, "mass", h, connectivity=conn)
            got, got_max = group.spatial(t[None], m, "mass", h, connectivity=conn)
            MEASURED["maps_compared"] += 1
            tally(got, want)
            where = (name, "mask" if m is not None else "no mask", conn)
            assert same(got, want), where
            assert same(got_max, want_max), where
            assert (got >= 0).all() and (m is None or (got[0][m == 0] == 0).all())
            # membership is the extent's
            assert np.array_equal(got > 0, group.spatial(t[None], m, "extent", h, connectivity=conn)[0] > 0), where
    if name == "nothing_above_the_threshold":
        assert not got.any() and got_max[0] == 0.0


def test_equal_sizes_and_different_heights(group):
    t = np.array([3.0, 3.5, 0.0, 6.0, 7.25, 1.0]).reshape(1, 1, 6)
    assert np.array_equal(group.cluster_mass(t, 2.0, connectivity=6).ravel(), [6.5, 6.5, 0.0, 13.25, 13.25, 0.0])
    assert np.array_equal(group.cluster_extent(t, 2.0, connectivity=6).ravel(), [2, 2, 0, 2, 2, 0])


# ---------------------------------------------------------------- the bits of a map depend on that map alone

@pytest.fixture(scope="module")
def batch(group):
    """max_k smooth maps at 9 x 8 x 7, their mask, the threshold, and the restatement"""
    maps = np.stack([smooth((9, 8, 7), 100 + k)[0] for k in range(MAX_K)])
    mask, h = random_mask((9, 8, 7), 99), 0.3
    want, want_max = cm.spatial(maps, mask, "mass", h, connectivity=18)
    assert (want > 0).any(axis=(1, 2, 3)).all()
    return maps, mask, h, want, want_max


def test_a_map_does_not_depend_on_k_place_or_mates(group, batch):
    maps, mask, h, want, want_max = batch
    for K in (1, 7, MAX_K):
        out, kmax = group.spatial(maps[:K], mask, "mass", h, connectivity=18)            # one launch of K maps
        assert same(out, want[:K]) and same(kmax, want_max[:K]), K
    order = np.random.default_rng(5).permutation(MAX_K)                                  # other places: kmax is permuted with the batch
    out2, kmax2 = group.spatial(maps[order], mask, "mass", h, connectivity=18)
    assert same(out2, want[order]) and same(kmax2, want_max[order])
    mates = np.concatenate([maps[3:4], np.full((6,) + maps.shape[1:], 7.0), -maps[:1]])  # other mates, K = 8
    out3, kmax3 = group.spatial(mates, mask, "mass", h, connectivity=18)
    assert same(out3[0], want[3]) and same(kmax3[:1], want_max[3:4]) and not out3[7][maps[0] > 0].any()
    small = group.tfce_work_bytes(5, maps.shape[1:])                                      # batches of 5: 7 launches
    out4, kmax4 = group.spatial(maps, mask, "mass", h, connectivity=18, work_bytes=small)
    assert same(out4, want) and same(kmax4, want_max)
    assert same(group.cluster_mass(maps[1], h, mask), cm.transform(maps[1], h, mask, 26))
    assert same(group.cluster_mass(maps[:3], h, mask, connectivity=6), cm.spatial(maps[:3], mask, "mass", h, connectivity=6)[0])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_mirrored_maps_give_mirrored_results(group, batch, axis):
    maps, mask, h, *_ = batch
    for conn in (6, 26):
        out, kmax = group.spatial(maps[:4], mask, "mass", h, connectivity=conn)
        flipped, kmax_f = group.spatial(np.flip(maps[:4], axis + 1), np.flip(mask, axis), "mass", h, connectivity=conn)
        assert same(np.flip(flipped, axis + 1), out) and same(kmax_f, kmax)


# ---------------------------------------------------------------- the group entries

GRID, N_MASK = (9, 8, 7), 300


def make_inputs(group, n, r, K, seed, f_rows=0):
    """300 voxels of the 9 x 8 x 7 grid with a smooth mean, so that components have some extent; f_rows = s: an F-contrast over the first s columns"""
    rng = np.random.default_rng([seed, n, r, K])
    X = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, r - 1))], axis=1)
    at = np.sort(rng.choice(int(np.prod(GRID)), N_MASK, replace=False)).astype(np.int32)
    mean = ndimage.uniform_filter(rng.standard_normal(GRID), 3).reshape(-1)[at] * 2.0 + 0.3
    Y = rng.standard_normal((n, N_MASK)) + mean[None, :]
    if f_rows:
        Cm = np.eye(r)[:, :f_rows]
        perms = group.permutation_set(X, Cm, K, seed, "flip")
        W, s, dof = group.weights_f(X, Cm, perms)
        Yr, s0 = group.residualise(Y, X, Cm)
        return Yr, s0, W, at, s, float(dof) / float(s)
    c = np.zeros(r)
    c[0] = 1.0
    perms = group.permutation_set(X, c, K, seed, "flip")
    W, _ = group.weights(X, c, perms)
    assert len(perms.index) == K
    Yr, s0 = group.residualise(Y, X, c)
    return Yr, s0, W, at


def check_entry(group, entry, stat_dev, want_stat, at, h, conn):
    """entry(ref, count, want_first, W rows) -> (kmax, count, first); stat_dev [K, V]: the device's own statistic, want_stat: the restatement's"""
    K = stat_dev.shape[0]
    assert same(stat_dev, want_stat)
    maps, mask = tn.dense(stat_dev, GRID, at)
    s_dev = group.cluster_mass(maps, h, mask, connectivity=conn).reshape(K, -1)[:, at]   # met2_tfce on the device's statistic maps
    want = cm.spatial(maps, mask, "mass", h, connectivity=conn)[0].reshape(K, -1)[:, at]
    assert same(s_dev, want) and (want[0] > 0).any()
    ref = want[0].copy()
    kmax, count, first = entry(ref, None, True, slice(None))
    tally(first, ref, True)
    tally(kmax, want.max(axis=1), True)
    assert same(first, ref) and same(kmax, want.max(axis=1))
    assert count.dtype == np.uint32 and np.array_equal(count, (want >= ref[None, :]).sum(axis=0))
    kmax2, none, none2 = entry(None, None, False, slice(None))
    assert none is None and none2 is None and same(kmax2, kmax)
    _, twice, _ = entry(ref, count, False, slice(None))                                  # count accumulates over two launches
    assert np.array_equal(twice, 2 * count)
    _, once, again = entry(ref, None, True, slice(0, 1))
    assert same(again, ref) and (once == 1).all()


@pytest.mark.parametrize("n,r", [(5, 1), (12, 2)])
def test_t_entry_equals_cluster_mass_of_the_t_maps_and_the_restatement(group, n, r):
    K = 7
    Y, s0, W, at = make_inputs(group, n, r, K, 60)
    t_dev = np.stack([group.perm_stats(Y, s0, W[k:k + 1], want_first=True)[2] for k in range(K)])
    entry = lambda ref, count, first, rows: group.perm_tfce(Y, s0, W[rows], GRID, at, "mass", 1.0, connectivity=26, ref=ref, count=count, want_first=first)
    check_entry(group, entry, t_dev, gn.perm_t(Y, s0, W)[0], at, 1.0, 26)
    got = cm.batch_spatial(Y, s0, W, GRID, at, "mass", 1.0, 0.5, 2.0, 26, None, True)
    assert same(got[0], entry(None, None, False, slice(None))[0])


def test_f_entry_equals_cluster_mass_of_the_f_maps_and_the_restatement(group):
    K = 7
    Y, s0, W, at, s, scale = make_inputs(group, 12, 3, K, 61, f_rows=2)
    assert s == 2
    f_dev = np.stack([group.perm_fstats(Y, s0, W[k:k + 1], s, scale, want_first=True)[2] for k in range(K)])
    entry = lambda ref, count, first, rows: group.perm_ftfce(Y, s0, W[rows], s, scale, GRID, at, "mass", 2.0, connectivity=18, ref=ref, count=count,
                                                             want_first=first)
    check_entry(group, entry, f_dev, gf.perm_f(Y, s0, W, s, scale)[0], at, 2.0, 18)


def test_pseudo_t_entry_equals_cluster_mass_of_the_pseudo_t_maps_and_the_restatement(group):
    K = 7
    Y, s0, W, at = make_inputs(group, 6, 1, K, 62)
    taps = group.smoothing_taps(1.0)[1]
    v_dev = np.stack([group.perm_vsm(Y, s0, W[k:k + 1], GRID, at, taps, "voxel", want_first=True)[2] for k in range(K)])
    entry = lambda ref, count, first, rows: group.perm_vsm(Y, s0, W[rows], GRID, at, taps, "mass", dh=1.0, connectivity=6, ref=ref, count=count,
                                                           want_first=first)
    check_entry(group, entry, v_dev, gv.perm_vt(Y, s0, W, GRID, at, taps), at, 1.0, 6)
    assert group.vsm_work_bytes(3, GRID, N_MASK, "mass") == group.vsm_work_bytes(3, GRID, N_MASK, "extent")


# ---------------------------------------------------------------- limits and refusals

def test_refusals_change_no_output(group, L):
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dt).contiguous()
    p = lambda x: None if x is None else x.data_ptr()
    i3 = lambda d: (C.c_int32 * 3)(*d)
    maps, out, kmax = t(np.ones((2, 4, 3, 2))), t(np.full((2, 4, 3, 2), 5.0)), t(np.full(2, 5.0))
    ok = dict(K=2, dims=(4, 3, 2), maps=maps, mask=None, mode=3, dh=0.5, E=0.5, H=2.0, conn=6, out=out, kmax=kmax)

    def tfce(**kw):
        a = dict(ok, **kw)
        return L.met2_tfce(0, a["K"], i3(a["dims"]), p(a["maps"]), p(a["mask"]), a["mode"], a["dh"], a["E"], a["H"], a["conn"], p(a["out"]),
                           p(a["kmax"]), None, 0, None)

    bad = [dict(dh=0.0), dict(dh=-1.0), dict(dh=float("nan")), dict(dh=float("inf")), dict(conn=8), dict(conn=0), dict(mode=2), dict(mode=4),
           dict(mode=-1), dict(K=0), dict(dims=(0, 3, 2)), dict(dims=(4, 3, -1)), dict(maps=None), dict(out=None), dict(out=maps)]
    for kw in bad:
        assert tfce(**kw) == INVALID and L.met2_last_error(), kw
    big = (257, 256, 256)                                          # one plane more than 2^24 voxels
    for kw in (dict(K=MAX_K + 1), dict(dims=big), dict(dims=big, maps=None), dict(dims=(2048, 1024, 1024))):
        assert tfce(**kw) == UNSUPPORTED and L.met2_last_error(), kw
    assert tfce(dims=big, maps=None, mode=1) == INVALID             # the extent gets past the size check, to the NULL pointer
    assert tfce(dims=(256, 256, 256), maps=None) == INVALID        # 2^24 itself is allowed in mass mode
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5.0).all() and (kmax.cpu().numpy() == 5.0).all()
    assert tfce(E=float("nan"), H=-1.0) == 0                        # the mass does not read E and H
    assert same(out.cpu().numpy(), np.full((2, 4, 3, 2), 24.0)) and same(kmax.cpu().numpy(), np.full(2, 24.0))
    assert tfce(kmax=None) == 0

    n, V = 5, 10
    Y, s0, W = t(np.ones((n, V))), t(np.full(V, 9.0)), t(np.ones((2, 2, n)))
    at, ref = t(np.arange(V) * 2, torch.int32), t(np.zeros(V))
    first, gmax, cnt = t(np.full(V, 5.0)), t(np.full(2, 5.0)), torch.full((V,), 7, dtype=torch.int32, device="cuda")
    gok = dict(n=n, V=V, Y=Y, s0=s0, r=1, K=2, W=W, dims=(4, 3, 2), at=at, mode=3, dh=0.5, conn=6, ref=ref, first=first, kmax=gmax, count=cnt, two=0)
    radius, one = i3((0, 0, 0)), (C.c_double * 1)(1.0)

    def grp_t(a):
        return L.met2_group_perm_tfce(0, a["n"], a["V"], p(a["Y"]), p(a["s0"]), a["r"], a["K"], p(a["W"]), i3(a["dims"]), p(a["at"]), a["mode"],
                                      a["dh"], 0.5, 2.0, a["conn"], p(a["ref"]), p(a["first"]), p(a["kmax"]), p(a["count"]), None, 0, None)

    def grp_f(a):
        return L.met2_group_perm_ftfce(0, a["n"], a["V"], p(a["Y"]), p(a["s0"]), a["r"], 1, 4.0, a["K"], p(a["W"][:, :1].contiguous()), i3(a["dims"]),
                                       p(a["at"]), a["mode"], a["dh"], 0.5, 2.0, a["conn"], p(a["ref"]), p(a["first"]), p(a["kmax"]), p(a["count"]),
                                       None, 0, None)

    def grp_v(a):
        return L.met2_group_perm_vsm(0, a["n"], a["V"], p(a["Y"]), p(a["s0"]), a["r"], a["K"], p(a["W"]), a["two"], i3(a["dims"]), p(a["at"]),
                                     a["mode"], a["dh"], 0.5, 2.0, a["conn"], radius, one, one, one, p(a["ref"]), p(a["first"]), p(a["kmax"]),
                                     p(a["count"]), None, 0, None)

    descending = t(np.arange(V)[::-1] * 2, torch.int32)
    for entry in (grp_t, grp_f, grp_v):
        for kw in bad[:5] + [dict(mode=4), dict(at=None), dict(kmax=None), dict(count=None), dict(V=25), dict(at=descending)]:
            assert entry(dict(gok, **kw)) == INVALID and L.met2_last_error(), (entry.__name__, kw)
        for kw in (dict(K=MAX_K + 1), dict(dims=big)):
            assert entry(dict(gok, **kw)) == UNSUPPORTED and L.met2_last_error(), (entry.__name__, kw)
    assert grp_v(dict(gok, two=1)) == INVALID and grp_t(dict(gok, mode=2)) == INVALID
    torch.cuda.synchronize()
    assert (first.cpu().numpy() == 5.0).all() and (gmax.cpu().numpy() == 5.0).all() and (cnt.cpu().numpy() == 7).all()
    for entry in (grp_t, grp_f, grp_v):
        before = cnt.cpu().numpy().copy()
        assert entry(gok) == 0 and (cnt.cpu().numpy() > before).all(), entry.__name__

    def bytes_of(mode):
        o = C.c_int64(-1)
        return L.met2_group_vsm_work_bytes(2, i3((4, 3, 2)), V, mode, C.byref(o)), o.value
    assert bytes_of(3) == bytes_of(1) and bytes_of(3)[0] == 0 and bytes_of(4)[0] == INVALID
    with pytest.raises(Exception):
        group.cluster_mass(np.ones((1, 1, 1)), 0.0)


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def planted(group):
    """the planted case of tests/test_cluster_mass_host.py with 64 of its sign flips, on the host with the stand-ins"""
    Y, X, c, grid, at, block, near = tn.planted_case()
    kw = dict(n_perm=64, seed=0, exchange="flip", cluster_mass_threshold=2.5, cluster_connectivity=26)
    host = group.randomise(Y, X, c, batch_stat=gn.batch_stat, batch_spatial=cm.batch_spatial, grid=grid, at=at, **kw)
    return Y, X, c, grid, at, block, near, kw, host


MASS_ARRAYS = ("cluster_mass", "p_mass_uncorrected", "p_mass_fwe", "mass_count", "mass_max_dist")


def test_randomise_and_the_filter_give_the_host_run(group, planted):
    motor = importlib.import_module(PKG + ".motor")
    Y, X, c, grid, at, block, near, kw, host = planted
    dev = group.randomise(Y, X, c, grid=grid, at=at, **kw)
    assert set(dev) == set(host)
    for key in host:
        assert np.array_equal(dev[key], host[key]), key
    assert same(dev["cluster_mass"], host["cluster_mass"]) and same(dev["mass_max_dist"], host["mass_max_dist"])
    tally(dev["cluster_mass"], host["cluster_mass"], True)
    tally(dev["mass_max_dist"], host["mass_max_dist"], True)
    out = motor.group_stats_filter(Y.reshape((Y.shape[0],) + grid), X, c, **kw)
    for key in ("tstat", "p_fwe", "count", "cluster_mass", "p_mass_uncorrected", "p_mass_fwe", "mass_count"):
        assert out[key].shape == grid and np.array_equal(out[key].reshape(-1), host[key]), key
    for key in ("max_dist", "mass_max_dist", "mass_crit", "t_crit", "cluster_mass_threshold", "cluster_connectivity"):
        assert np.array_equal(out[key], host[key]), key
    # a small work space: more, smaller batches, the same bits; and without the option nothing of the mass appears
    again = group.randomise(Y, X, c, grid=grid, at=at, work_bytes=group.tfce_work_bytes(3, grid, Y.shape[1]), **kw)
    assert np.array_equal(again["mass_count"], dev["mass_count"]) and same(again["mass_max_dist"], dev["mass_max_dist"])
    plain = group.randomise(Y, X, c, **{k: kw[k] for k in ("n_perm", "seed", "exchange")})
    assert not [k for k in plain if "mass" in k] and all(np.array_equal(plain[k], dev[k]) for k in plain)
    # the fixed point against the long double sum of the device's own t maps
    Yr, s0 = group.residualise(Y, X, c)
    t_maps = gn.perm_t(Yr, s0, group.weights(X, c, group.permutation_set(X, c, 8, 0, "flip"))[0])[0].reshape((8,) + grid)
    assert np.array_equal(t_maps[0].reshape(-1), dev["tstat"])
    got = group.cluster_mass(t_maps, 2.5)
    for k in range(8):
        exact, e = cm.exact_sum(t_maps[k], 2.5)
        live = e > 0
        err = np.abs(got[k].astype(np.longdouble) - exact)[live].astype(np.float64)
        ratio = err / (e[live] * 2.0 ** -25)
        assert live.any() and (err <= (e[live] * 2.0 ** -25 + np.spacing(got[k][live]) / 2) * (1 + 1e-3)).all()
        MEASURED["worst_error_over_e_2^-25"] = max(MEASURED["worst_error_over_e_2^-25"], float(ratio.max()))
    print("worst |out - exact| / (e 2^-25) on the planted case's maps: %.4f" % MEASURED["worst_error_over_e_2^-25"])


def test_f_and_pseudo_t_paths_of_randomise_give_the_host_run(group):
    rng = np.random.default_rng(21)
    grid = (5, 4, 3)
    at = np.sort(rng.choice(60, 50, replace=False))
    X, fc = gf.three_group_design((3, 3, 3), covariate=False)
    Y = rng.standard_normal((9, 50))
    Y[3:6, :20] += 2.0
    kw = dict(n_perm=40, seed=1, grid=grid, at=at)
    host = group.randomise(Y, X, f_contrast=fc, batch_stat=gf.batch_stat, batch_spatial=cm.batch_spatial_f, cluster_mass_threshold=3.0,
                           cluster_connectivity=18, **kw)
    dev = group.randomise(Y, X, f_contrast=fc, cluster_mass_threshold=3.0, cluster_connectivity=18, **kw)
    assert set(dev) == set(host) and (host["cluster_mass"] > 0).any()
    for key in host:
        assert np.array_equal(dev[key], host[key]), key
    X1, c = gn.one_sample_design(9)
    host = group.randomise(Y + 0.5, X1, c, exchange="flip", batch_stat=gn.batch_stat, batch_spatial=cm.batch_spatial_vsm, variance_smoothing=1.0,
                           cluster_mass_threshold=1.0, **kw)
    dev = group.randomise(Y + 0.5, X1, c, exchange="flip", variance_smoothing=1.0, cluster_mass_threshold=1.0, **kw)
    assert set(dev) == set(host) and (host["cluster_mass"] > 0).any()
    for key in host:
        assert np.array_equal(dev[key], host[key]), key


def test_driver_writes_the_mass_files(group, tmp_path):
    motor = importlib.import_module(PKG + ".motor")
    nifti = importlib.import_module(PKG + ".nifti")
    rng = np.random.default_rng(61)
    shape, n = (8, 7, 5), 8
    affine = np.diag([2.0, 2.0, 3.0, 1.0])
    X, c = gn.one_sample_design(n)
    inside = np.ones(shape, dtype=np.uint8)
    inside[0], inside[:, 0] = 0, 0                                 # the tested voxels' bounding box is smaller than the grid
    paths, vols = [], []
    for i in range(n):
        vol = rng.standard_normal(shape) + 0.2
        vol[3:6, 2:5, 1:4] += 1.2
        path = str(tmp_path / ("s%02d_" % i))
        nifti.save(nifti.NiftiImage(vol, affine), path + "MWF_in_template.nii.gz")
        nifti.save(nifti.NiftiImage(inside, affine), path + "maps_to_template_inside.nii.gz")
        paths.append(path)
        vols.append(vol)
    out_path = str(tmp_path / "group_")
    out = motor.motor_group_stats(paths, "MWF", X, c, out_path, n_perm=64, seed=1, exchange="flip", cluster_mass_threshold=2.0, cluster_connectivity=18)
    at = np.flatnonzero(inside.reshape(-1))
    host = group.randomise(np.stack(vols).reshape(n, -1)[:, at], X, c, n_perm=64, seed=1, exchange="flip", batch_stat=gn.batch_stat,
                           batch_spatial=cm.batch_spatial, cluster_mass_threshold=2.0, cluster_connectivity=18, grid=shape, at=at)
    for key, name in (("cluster_mass", "cluster_mass"), ("p_mass_fwe", "p_mass_fwe"), ("tstat", "tstat")):
        img = nifti.load(out_path + "MWF_" + name + ".nii.gz")
        got = img.get_fdata().reshape(-1)
        assert np.allclose(img.affine, affine) and np.array_equal(got[at], host[key]) and np.array_equal(got, out[key].reshape(-1)), key
        assert (got[inside.reshape(-1) == 0] == (1.0 if key.startswith("p_") else 0.0)).all()
    assert out["mass_count"].shape == shape and np.array_equal(out["mass_count"].reshape(-1)[at], host["mass_count"])
    assert np.array_equal(np.loadtxt(out_path + "MWF_mass_max_dist.txt"), host["mass_max_dist"])
    report = open(out_path + "MWF_group_report.txt").read()
    assert "cluster mass: threshold = 2, connectivity = 18" in report and "%.6f" % host["mass_crit"] in report
    assert "p_mass_fwe <= 0.05: %d" % int((host["p_mass_fwe"] <= 0.05).sum()) in report and (host["cluster_mass"] > 0).any()
    assert not os.path.exists(out_path + "MWF_cluster_extent.nii.gz")
