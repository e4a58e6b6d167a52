"""met2_tfce and met2_group_perm_tfce on the device (include/met2_hip.h states the definitions) against their numpy restatement
(tests/tools/tfce_numpy.py: scipy.ndimage.label per level, independent of union-find), and group_stats_filter / motor_group_stats end to end
against the host run of the planted case of tests/test_tfce_host.py.
Equality.  The header fixes the level rule, the order of the sum and forbids fused products, and for E = 0.5, H = 2 a term is a correctly
rounded square root times a square: the device's out and kmax must EQUAL the float64 restatement bit for bit, for TFCE and for the extent, at
connectivity 6, 18 and 26, with and without a mask, on every case of CASES.  Before any device call each case asserts on the restatement that it
has the structure it is named for.  The same from the device alone: a map's bits do not depend on K, its place, its batch mates or the
number of batches; mirrored maps give mirrored results; a permuted batch permutes kmax.
Group entry.  first, kmax and count EQUAL met2_tfce applied to the t maps that met2_group_perm_stats returns one candidate at a time, and the
restatement.  Before that the long-double restatement asserts that no candidate's statistic lies within 1e-10 max of the observed one at a
voxel unless the two are exactly equal there (both 0 outside every support, the same integer extent, or the same levels around the voxel,
which give the same terms: equal in every precision), so no comparison s >= ref hangs on a rounding.
Accuracy for general exponents (E = 0.6, H = 1.5: pow).  max |out - long double| / max |long double| <= 16 x the largest such figure measured on
an MI355X over these very cases (profiles/tfce_parity.json), which may not exceed 1e-12: float64 numpy's own figure on the same cases is
asserted below 1e-14, so more would be a defect, not rounding.  With MET2_TFCE_PARITY_OUT=<file> the module writes what it measured there."""
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
import group_numpy as gn                                           # noqa: E402
import tfce_numpy as tn                                            # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
CEILING = 1e-12
MEASURED = {"tfce_pow": 0.0}
INVALID, UNSUPPORTED = -1, -2
LD = np.longdouble
MAX_K, MAX_STEPS = 32, 1024                                        # met2_tfce_limits (asserted below)
CONN = (6, 18, 26)


@pytest.fixture(scope="module")
def group():
    g = importlib.import_module(PKG + ".group")
    assert g.tfce_limits() == {"max_k": MAX_K, "max_steps": MAX_STEPS} and tn.MAX_STEPS == MAX_STEPS
    yield g
    path = os.environ.get("MET2_TFCE_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"max_rel_error": MEASURED, "reference": "tests/tools/tfce_numpy.py in long double, E = 0.6, H = 1.5",
                       "measure": "max |error| / max |reference| per case", "bound_factor": 16, "ceiling": CEILING,
                       "device": torch.cuda.get_device_name(0)}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib").lib()


def held(quantity, got, want):
    """records max |got - want| / max |want| for `quantity`, prints it, and holds it to the bound"""
    want = np.asarray(want, dtype=LD)
    err = float(np.abs(np.asarray(got, dtype=LD) - want).max() / np.abs(want).max())
    MEASURED[quantity] = max(MEASURED[quantity], err)
    print("%s: relative error %.3g" % (quantity, err))
    path = os.path.join(ROOT, "profiles", "tfce_parity.json")
    assert os.path.exists(path), "%s is missing: it holds the measured figures the bounds derive from" % path
    b = 16.0 * float(json.load(open(path))["max_rel_error"][quantity])
    assert 0.0 < b <= CEILING, "the measured error of %s puts the bound at %g: above %g it is a defect, not rounding" % (quantity, b, CEILING)
    assert err <= b, (quantity, err, b)


# ---------------------------------------------------------------- the cases: name -> (t [nx, ny, nz], dh, mask or None, extent threshold)

def ncomp(t, dh, conn, mask=None, mode="tfce"):
    return tn.transform(t, mask, mode, dh, connectivity=conn)[1]


def random_mask(shape, seed):
    return (np.random.default_rng(seed).random(shape) < 0.8).astype(np.uint8)


def line(shape, seed):
    t = np.random.default_rng(seed).standard_normal(shape) * 1.5 + 0.5
    return t, 0.25, random_mask(shape, seed + 1), 1.0


def row_ends(shape):
    """voxels that follow each other in memory across the end of a row (z), of a plane (y) and nowhere else: none are neighbours under 6"""
    nx, ny, nz = shape
    t = np.zeros(shape)
    for x in range(0, nx - 1, 4):
        t[x, 0, nz - 1], t[x, 1, 0] = 2.0, 2.0                     # linear neighbours across a row end
        t[x, ny - 1, nz - 1], t[x + 1, 0, 0] = 2.0, 2.0            # ... across a plane end
    lit = int((t > 0).sum())
    assert ncomp(t, 1.0, 6)[1] == lit, "the lit voxels must all be isolated under connectivity 6"
    assert ncomp(t, 1.0, 26)[1] < lit
    return t, 1.0, None, 1.5


def serpentine(flat):
    """a 6-connected path through all of 16 x 16 x 4; with the gradient, level j holds the path's first 1 025 - j voxels: one more per level"""
    shape, order, i = (16, 16, 4), np.zeros((16, 16, 4), dtype=np.int64), 0
    prev = None
    for x in range(16):
        for yi in range(16):
            y = yi if x % 2 == 0 else 15 - yi
            for zi in range(4):
                z = zi if (x * 16 + yi) % 2 == 0 else 3 - zi
                if prev is not None:
                    assert abs(prev[0] - x) + abs(prev[1] - y) + abs(prev[2] - z) == 1
                prev = (x, y, z)
                order[x, y, z] = i
                i += 1
    if flat:
        t, dh = np.full(shape, 1.0), 1.0 / 3.0
        assert list(ncomp(t, dh, 6)[1:]) == [1, 1, 1]
    else:
        t, dh = (1024 - order) * 0.5, 0.5
        lev = tn.levels(t, dh)
        assert lev.max() == MAX_STEPS and lev.min() == 1 and len(np.unique(lev)) == 1024
        assert (ncomp(t, dh, 6)[1:] == 1).all()
    return t, dh, None, 0.75 if flat else 100.25


def checkerboard():
    x, y, z = np.indices((8, 7, 5))
    t = np.where((x + y + z) % 2 == 0, 2.0, 0.0)
    lit = int((t > 0).sum())
    assert ncomp(t, 1.0, 6)[2] == lit and ncomp(t, 1.0, 18)[2] == 1 and ncomp(t, 1.0, 26)[2] == 1
    return t, 1.0, None, 1.0


def bridge():
    t = np.zeros((9, 5, 3))
    t[0:3, 1:4, :] = 3.0
    t[6:9, 1:4, :] = 2.5
    t[3:6, 2, 1] = 1.0                                             # the bridge: level 1 only
    assert list(ncomp(t, 1.0, 6)[1:]) == [1, 2, 1]
    return t, 1.0, None, 2.0


def wall():
    t = np.full((9, 5, 3), 2.0)
    mask = np.ones((9, 5, 3), dtype=np.uint8)
    mask[4] = 0
    for conn in CONN:
        assert list(ncomp(t, 1.0, conn, mask)[1:]) == [2, 2] and list(ncomp(t, 1.0, conn)[1:]) == [1, 1]
    return t, 1.0, mask, 1.0


def plateaus():
    """values exactly on a threshold j dh, and one ulp below it"""
    rng = np.random.default_rng(31)
    j = rng.integers(0, 7, (7, 6, 5))
    dh = 0.3
    on = j.astype(np.float64) * dh
    below = rng.random(j.shape) < 0.5
    t = np.where(below & (j > 0), np.nextafter(on, -np.inf), on)
    assert np.array_equal(tn.levels(t, dh), np.where(below & (j > 0), j - 1, j)) and (below & (j > 0)).sum() > 20
    return t, dh, random_mask(j.shape, 32), np.float64(3) * dh


def nothing_positive():
    t = -np.abs(np.random.default_rng(33).standard_normal((5, 4, 3)))
    t[0, 0, 0] = 0.0
    assert tn.levels(t, 0.1).max() == 0
    return t, 0.1, None, 0.1


def odd_values():
    t = np.random.default_rng(34).standard_normal((6, 5, 4)) + 1.0
    t[0, 0, 0], t[1, 2, 3], t[2, 2, 2], t[3, 1, 0], t[5, 4, 3] = -0.0, np.nan, -np.inf, np.nan, -0.0
    lev = tn.levels(t, 0.2)
    assert lev[1, 2, 3] == 0 and lev[2, 2, 2] == 0 and lev[0, 0, 0] == 0 and lev.max() > 5
    return t, 0.2, random_mask(t.shape, 35), 1.0


def clamp():
    t = np.random.default_rng(36).random((4, 4, 4)) * 5.0
    t[1, 1, 1] = np.inf
    dh = 0.004
    assert (t[np.isfinite(t)] / dh > MAX_STEPS + 1).sum() > 5 and tn.levels(t, dh).max() == MAX_STEPS
    return t, dh, None, 3.0


def smooth(shape, seed):
    t = ndimage.uniform_filter(np.random.default_rng(seed).standard_normal(shape), 3, mode="constant") * 3.0
    return t, float(t.max()) / 100.0, random_mask(shape, seed + 1), float(t.max()) / 3.0


CASES = {"1x1x1": lambda: (np.full((1, 1, 1), 3.2), 1.0, None, 2.0)}
for _n in (2, 64, 65, 257):
    CASES["line_z_%d" % _n] = lambda n=_n: line((1, 1, n), n)
    CASES["line_x_%d" % _n] = lambda n=_n: line((n, 1, 1), n + 300)
    CASES["line_y_%d" % _n] = lambda n=_n: line((1, n, 1), n + 600)
CASES.update({
    "row_ends_65x3x2": lambda: row_ends((65, 3, 2)), "row_ends_3x65x2": lambda: row_ends((3, 65, 2)),
    "random_65x3x2": lambda: smooth((65, 3, 2), 41), "random_3x65x2": lambda: smooth((3, 65, 2), 43),
    "serpentine_gradient": lambda: serpentine(False), "serpentine_flat": lambda: serpentine(True),
    "checkerboard": checkerboard, "bridge_at_level_1": bridge, "wall_of_mask_zeros": wall, "plateaus_and_one_ulp_below": plateaus,
    "nothing_positive": nothing_positive, "minus_zero_nan_minus_inf": odd_values, "clamp_at_max_steps": clamp,
    "smooth_33x17x9": lambda: smooth((33, 17, 9), 45),
})


@pytest.mark.parametrize("name", sorted(CASES))
def test_out_and_kmax_equal_the_float64_restatement(group, name):
    t, dh, mask, h = CASES[name]()
    for m in ((None,) if mask is None else (None, mask)):
        for conn in CONN:
            for mode, step in (("tfce", dh), ("extent", h)):
                want, want_max = tn.spatial(t[None], m, mode, step, connectivity=conn)
                got, got_max = group.spatial(t[None], m, mode, step, connectivity=conn)
                where = (name, "mask" if m is not None else "no mask", conn, mode)
                assert np.array_equal(got, want), where
                assert np.array_equal(got_max, want_max), where
                assert (got >= 0).all() and (m is None or (got[0][m == 0] == 0).all())


# ---------------------------------------------------------------- the bits of a map depend on that map alone

@pytest.fixture(scope="module")
def batch(group):
    """max_k smooth maps at 9 x 8 x 7, their mask, dh, and the device's result for each map on its own (K = 1)"""
    maps = np.stack([smooth((9, 8, 7), 100 + k)[0] for k in range(MAX_K)])
    mask, dh = random_mask((9, 8, 7), 99), 0.02
    assert tn.levels(maps, dh).max() > 40
    alone = [group.spatial(maps[k:k + 1], mask, "tfce", dh, connectivity=18) for k in range(MAX_K)]
    return maps, mask, dh, np.concatenate([a[0] for a in alone]), np.concatenate([a[1] for a in alone])


def test_a_map_does_not_depend_on_k_place_mates_or_batches(group, batch):
    maps, mask, dh, alone, alone_max = batch
    assert np.array_equal(alone, tn.spatial(maps, mask, "tfce", dh, connectivity=18)[0])
    out, kmax = group.spatial(maps, mask, "tfce", dh, connectivity=18)                 # one launch of max_k
    assert np.array_equal(out, alone) and np.array_equal(kmax, alone_max)
    order = np.random.default_rng(5).permutation(MAX_K)                                # other places: kmax is permuted with the batch
    out2, kmax2 = group.spatial(maps[order], mask, "tfce", dh, connectivity=18)
    assert np.array_equal(out2, alone[order]) and np.array_equal(kmax2, alone_max[order])
    mates = np.concatenate([maps[3:4], np.full((6,) + maps.shape[1:], 7.0), -maps[:1]])  # other mates, K = 8
    out3, kmax3 = group.spatial(mates, mask, "tfce", dh, connectivity=18)
    assert np.array_equal(out3[0], alone[3]) and kmax3[0] == alone_max[3]
    small = group.tfce_work_bytes(5, maps.shape[1:])                                     # batches of 5: 7 launches
    out4, kmax4 = group.spatial(maps, mask, "tfce", dh, connectivity=18, work_bytes=small)
    assert group._batch_for(maps.shape[1:], 0, small, MAX_K) == 5 and np.array_equal(out4, alone) and np.array_equal(kmax4, alone_max)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_mirrored_maps_give_mirrored_results(group, batch, axis):
    maps, mask, dh, *_ = batch
    for mode, step, conn in (("tfce", dh, 6), ("extent", 0.5, 26)):
        out, kmax = group.spatial(maps[:4], mask, mode, step, connectivity=conn)
        flipped, kmax_f = group.spatial(np.flip(maps[:4], axis + 1), np.flip(mask, axis), mode, step, connectivity=conn)
        assert np.array_equal(np.flip(flipped, axis + 1), out) and np.array_equal(kmax_f, kmax)


def test_module_level_functions(group, batch):
    maps, mask, dh, *_ = batch
    filters = importlib.import_module(PKG + ".filters")
    top = maps[0][mask != 0].max()
    want = tn.transform(maps[0], mask, "tfce", top / 100.0)[0]
    assert np.array_equal(group.tfce(maps[0], mask), want) and np.array_equal(filters.tfce_filter(maps[0], mask), want)
    assert np.array_equal(group.tfce(maps[:3], mask, dh=dh, connectivity=26), tn.spatial(maps[:3], mask, "tfce", dh, connectivity=26)[0])
    assert np.array_equal(group.cluster_extent(maps[1], 0.4, mask), tn.transform(maps[1], mask, "extent", 0.4, connectivity=26)[0])
    assert not group.tfce(-np.abs(maps[0])).any()


# ---------------------------------------------------------------- general exponents: an accuracy bound

@pytest.mark.parametrize("name", ["smooth_33x17x9", "serpentine_gradient", "clamp_at_max_steps", "bridge_at_level_1", "line_z_257"])
def test_general_exponents_to_the_bound(group, name):
    t, dh, mask, _ = CASES[name]()
    ld = tn.transform(t, mask, "tfce", dh, E=0.6, H=1.5, dtype=LD)[0]
    f64 = tn.transform(t, mask, "tfce", dh, E=0.6, H=1.5)[0]
    own = float(np.abs(f64.astype(LD) - ld).max() / np.abs(ld).max())
    print("float64 numpy's own relative error: %.3g" % own)
    assert own <= 1e-14, "rounding alone costs numpy %g on this case" % own
    got = group.spatial(t[None], mask, "tfce", dh, E=0.6, H=1.5)[0][0]
    assert np.array_equal(got == 0, ld == 0)
    held("tfce_pow", got, ld)


# ---------------------------------------------------------------- the group entry

GRID, N_MASK = (9, 8, 7), 300


def make_inputs(group, n, r, K, seed):
    """test_gpu_group.py's inputs on 300 voxels of the 9 x 8 x 7 grid, with a smooth mean so that supports have some extent"""
    rng = np.random.default_rng([seed, n, r, K])
    X = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, r - 1))], axis=1)
    c = np.zeros(r)
    c[0] = 1.0
    perms = group.permutation_set(X, c, K, seed, "flip")
    assert len(perms.index) == K
    W, _ = group.weights(X, c, perms)
    at = np.sort(rng.choice(int(np.prod(GRID)), N_MASK, replace=False)).astype(np.int32)
    mean = ndimage.uniform_filter(rng.standard_normal(GRID), 3).reshape(-1)[at] * 2.0 + 0.3
    Yr, s0 = group.residualise(rng.standard_normal((n, N_MASK)) + mean[None, :], X, c)
    return Yr, s0, W, at


@pytest.mark.parametrize("K", [1, 7, MAX_K])
@pytest.mark.parametrize("n,r", [(5, 1), (5, 2), (12, 1), (12, 2)])
def test_group_entry_equals_tfce_of_the_t_maps_and_the_restatement(group, n, r, K):
    Y, s0, W, at = make_inputs(group, n, r, K, 50 + K)
    # the device's own t, one candidate at a time through t_first
    t_dev = np.stack([group.perm_stats(Y, s0, W[k:k + 1], want_first=True)[2] for k in range(K)])
    assert np.array_equal(t_dev, gn.perm_t(Y, s0, W)[0])
    maps, mask = tn.dense(t_dev, GRID, at)
    dh = float(t_dev[0].max()) / 100.0
    assert dh > 0
    for mode, step, conn in (("tfce", dh, 6), ("extent", 1.0, 26)):
        ld = tn.perm_spatial(Y, s0, W, GRID, at, mode, step, 0.5, 2.0, conn, None, LD)["s"]
        gap = np.abs(ld[1:] - ld[0][None, :])
        assert not ((gap > 0) & (gap <= 1e-10 * np.abs(ld).max())).any(), "a candidate's statistic lies within rounding of the observed one"
        s_dev = group.spatial(maps, mask, mode, step, connectivity=conn)[0].reshape(K, -1)[:, at]      # met2_tfce on the device's t maps
        ref = s_dev[0].copy()
        kmax, count, first = group.perm_tfce(Y, s0, W, GRID, at, mode, step, connectivity=conn, ref=ref, want_first=True)
        assert np.array_equal(first, ref) and np.array_equal(kmax, s_dev.max(axis=1))
        assert count.dtype == np.uint32 and np.array_equal(count, (s_dev >= ref[None, :]).sum(axis=0))
        want = tn.perm_spatial(Y, s0, W, GRID, at, mode, step, 0.5, 2.0, conn, ref)
        assert np.array_equal(s_dev, want["s"]) and np.array_equal(kmax, want["kmax"]) and np.array_equal(count, want["count"])
        assert np.array_equal(count, (ld >= ld[0][None, :]).sum(axis=0))               # the long-double restatement counts the same candidates
        # ref NULL: no count; first NULL: the same kmax; count accumulates
        kmax2, none, none2 = group.perm_tfce(Y, s0, W, GRID, at, mode, step, connectivity=conn)
        assert none is None and none2 is None and np.array_equal(kmax2, kmax)
        _, twice, _ = group.perm_tfce(Y, s0, W, GRID, at, mode, step, connectivity=conn, ref=ref, count=count)
        assert np.array_equal(twice, 2 * count)
        # the identity's own result fed back counts every voxel once
        _, once, again = group.perm_tfce(Y, s0, W[:1], GRID, at, mode, step, connectivity=conn, ref=ref, want_first=True)
        assert np.array_equal(again, ref) and (once == 1).all()


# ---------------------------------------------------------------- limits and refusals

def test_refusals_change_no_output(group, L):
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dt).contiguous()
    p = lambda x: None if x is None else x.data_ptr()
    i3 = lambda d: (C.c_int32 * 3)(*d)
    maps, out, kmax = t(np.ones((2, 4, 3, 2))), t(np.full((2, 4, 3, 2), 5.0)), t(np.full(2, 5.0))
    ok = dict(K=2, dims=(4, 3, 2), maps=maps, mask=None, mode=0, dh=0.5, E=0.5, H=2.0, conn=6, out=out, kmax=kmax)

    def tfce(**kw):
        a = dict(ok, **kw)
        return L.met2_tfce(0, a["K"], i3(a["dims"]), p(a["maps"]), p(a["mask"]), a["mode"], a["dh"], a["E"], a["H"], a["conn"], p(a["out"]),
                           p(a["kmax"]), None, 0, None)

    bad = [dict(dh=0.0), dict(dh=-1.0), dict(dh=float("nan")), dict(dh=float("inf")), dict(E=0.0), dict(E=-0.5), dict(E=float("nan")),
           dict(E=float("inf")), dict(H=-1.0), dict(H=float("nan")), dict(conn=8), dict(conn=0), dict(mode=2), dict(K=0), dict(dims=(0, 3, 2)),
           dict(dims=(4, 3, -1)), dict(maps=None), dict(out=None), dict(out=maps)]
    for kw in bad:
        assert tfce(**kw) == INVALID and L.met2_last_error(), kw
    for kw in (dict(K=MAX_K + 1), dict(dims=(2048, 1024, 1024)), dict(dims=(65536, 65536, 65536))):
        assert tfce(**kw) == UNSUPPORTED and L.met2_last_error(), kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5.0).all() and (kmax.cpu().numpy() == 5.0).all()
    assert tfce(mode=1, E=float("nan"), H=-1.0) == 0                                # the extent does not read E and H
    assert tfce() == 0 and np.array_equal(out.cpu().numpy(), tn.spatial(np.ones((2, 4, 3, 2)), None, "tfce", 0.5)[0])
    assert tfce(kmax=None) == 0

    n, V = 5, 10
    Y, s0, W = t(np.ones((n, V))), t(np.full(V, 9.0)), t(np.ones((2, 2, n)))
    at, ref = t(np.arange(V) * 2, torch.int32), t(np.zeros(V))
    first, gmax, cnt = t(np.full(V, 5.0)), t(np.full(2, 5.0)), torch.full((V,), 7, dtype=torch.int32, device="cuda")
    gok = dict(n=n, V=V, Y=Y, s0=s0, r=1, K=2, W=W, dims=(4, 3, 2), at=at, mode=0, dh=0.5, E=0.5, H=2.0, conn=6, ref=ref, first=first, kmax=gmax,
               count=cnt)

    def grp(**kw):
        a = dict(gok, **kw)
        return L.met2_group_perm_tfce(0, a["n"], a["V"], p(a["Y"]), p(a["s0"]), a["r"], a["K"], p(a["W"]), i3(a["dims"]), p(a["at"]), a["mode"],
                                      a["dh"], a["E"], a["H"], a["conn"], p(a["ref"]), p(a["first"]), p(a["kmax"]), p(a["count"]), None, 0, None)

    descending = t(np.arange(V)[::-1] * 2, torch.int32)
    repeated = t(np.minimum(np.arange(V), 8), torch.int32)
    beyond = t(np.arange(V) + 20, torch.int32)
    for kw in bad[:16] + [dict(Y=None), dict(s0=None), dict(W=None), dict(at=None), dict(kmax=None), dict(count=None), dict(r=0), dict(n=1),
                          dict(V=0), dict(V=25), dict(at=descending), dict(at=repeated), dict(at=beyond)]:
        assert grp(**kw) == INVALID and L.met2_last_error(), kw
    for kw in (dict(K=MAX_K + 1), dict(n=129), dict(r=9, n=20)):
        assert grp(**kw) == UNSUPPORTED and L.met2_last_error(), kw
    torch.cuda.synchronize()
    assert (first.cpu().numpy() == 5.0).all() and (gmax.cpu().numpy() == 5.0).all() and (cnt.cpu().numpy() == 7).all()
    assert grp() == 0 and (cnt.cpu().numpy() > 7).all()


def test_refused_group_calls_left_the_outputs(group, L):
    """the same refusals as above on fresh outputs, read back: nothing was written"""
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dt).contiguous()
    n, V = 5, 10
    Y, s0, W = t(np.ones((n, V))), t(np.full(V, 9.0)), t(np.ones((2, 2, n)))
    ref, first, gmax = t(np.zeros(V)), t(np.full(V, 5.0)), t(np.full(2, 5.0))
    cnt = torch.full((V,), 7, dtype=torch.int32, device="cuda")
    dims = (C.c_int32 * 3)(4, 3, 2)
    for at, dh, conn in ((t(np.arange(V)[::-1] * 2, torch.int32), 0.5, 6), (t(np.arange(V) + 20, torch.int32), 0.5, 6),
                         (t(np.arange(V), torch.int32), 0.0, 6), (t(np.arange(V), torch.int32), 0.5, 7)):
        rc = L.met2_group_perm_tfce(0, n, V, Y.data_ptr(), s0.data_ptr(), 1, 2, W.data_ptr(), dims, at.data_ptr(), 0, dh, 0.5, 2.0, conn,
                                    ref.data_ptr(), first.data_ptr(), gmax.data_ptr(), cnt.data_ptr(), None, 0, None)
        assert rc == INVALID
    torch.cuda.synchronize()
    assert (first.cpu().numpy() == 5.0).all() and (gmax.cpu().numpy() == 5.0).all() and (cnt.cpu().numpy() == 7).all()
    with pytest.raises(ValueError):
        group.spatial(np.ones((1, 2, 2, 2)), np.ones((2, 2, 3)), "tfce", 0.5)
    with pytest.raises(ValueError):
        group.perm_tfce(np.ones((4, 3)), np.ones(3), np.ones((1, 2, 4)), (2, 2, 2), np.arange(2), dh=0.5)


# ---------------------------------------------------------------- end to end

def test_group_stats_filter_gives_the_host_run(group):
    motor = importlib.import_module(PKG + ".motor")
    Y, X, c, grid, at, block, near, host = tn.planted_host(group)
    out = motor.group_stats_filter(Y.reshape((Y.shape[0],) + grid), X, c, n_perm=400, seed=0, exchange="flip", tfce=True, cluster_threshold=2.5)
    for key in ("tstat", "p_fwe", "count", "tfce", "p_tfce_uncorrected", "p_tfce_fwe", "tfce_count", "cluster_extent", "p_cluster_uncorrected",
                "p_cluster_fwe", "cluster_count"):
        assert out[key].shape == grid and np.array_equal(out[key].reshape(-1), host[key]), key
    for key in ("max_dist", "tfce_max_dist", "cluster_max_dist", "dh", "tfce_crit", "cluster_crit", "t_crit"):
        assert np.array_equal(out[key], host[key]), key
    found = out["p_tfce_fwe"].reshape(-1) <= 0.05
    assert found[block].sum() >= 72 and not found[~near].any()
    # a small work space: more, smaller batches, the same bits
    again = motor.group_stats_filter(Y.reshape((Y.shape[0],) + grid), X, c, n_perm=400, seed=0, exchange="flip", tfce=True,
                                     work_bytes=group.tfce_work_bytes(3, grid, Y.shape[1]))
    assert np.array_equal(again["tfce_count"], out["tfce_count"]) and np.array_equal(again["tfce_max_dist"], out["tfce_max_dist"])


def test_driver_writes_the_spatial_files(group, tmp_path):
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
    out = motor.motor_group_stats(paths, "MWF", X, c, out_path, n_perm=64, seed=1, exchange="flip", tfce={"connectivity": 18}, cluster_threshold=2.0)
    at = np.flatnonzero(inside.reshape(-1))
    host = group.randomise(np.stack(vols).reshape(n, -1)[:, at], X, c, n_perm=64, seed=1, exchange="flip", batch_stat=gn.batch_stat,
                           batch_spatial=tn.batch_spatial, tfce={"connectivity": 18}, cluster_threshold=2.0, grid=shape, at=at)
    for key, name in (("tfce", "tfce"), ("p_tfce_uncorrected", "p_tfce_unc"), ("p_tfce_fwe", "p_tfce_fwe"), ("cluster_extent", "cluster_extent"),
                      ("p_cluster_fwe", "p_cluster_fwe"), ("tstat", "tstat")):
        img = nifti.load(out_path + "MWF_" + name + ".nii.gz")
        got = img.get_fdata().reshape(-1)
        assert np.allclose(img.affine, affine) and np.array_equal(got[at], host[key]) and np.array_equal(got, out[key].reshape(-1)), key
        assert (got[inside.reshape(-1) == 0] == (1.0 if key.startswith("p_") else 0.0)).all()
    assert np.array_equal(np.loadtxt(out_path + "MWF_tfce_max_dist.txt"), host["tfce_max_dist"])
    report = open(out_path + "MWF_group_report.txt").read()
    assert "dh = %.6g, E = 0.5, H = 2, connectivity = 18" % host["dh"] in report and "%.6f" % host["tfce_crit"] in report
    assert "p_tfce_fwe <= 0.05: %d" % int((host["p_tfce_fwe"] <= 0.05).sum()) in report and "p_cluster_fwe <= 0.05" in report
    assert (host["p_tfce_fwe"] <= 0.05).sum() > 0
