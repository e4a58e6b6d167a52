"""met2_masked_smooth and met2_group_perm_vsm on the device (include/met2_hip.h states the definitions) against their float64 numpy restatement
(tests/tools/group_vsm_numpy.py, itself checked by tests/test_group_vsm_host.py), and group_stats_filter(variance_smoothing=...) end to end
against the host run of the planted small-sample case.
Equality.  The header fixes the order of every sum, forbids fused products and takes the taps from the host; division and square root are
correctly rounded: S, N, the pseudo-t, kmax, first and count must EQUAL the restatement bit for bit -- at every axis length against every
radius, on both sides of the smoothing kernel's tile extents (met2_group_vsm_limits), of the t kernel's voxel tile and of its candidate
groups, with masks that have holes, one voxel or none, for K = 1 and 32, one- and two-sided, and through TFCE and the cluster extent.
From the device alone: a map's bits do not depend on K, its place or its batch mates; what lies outside the mask is not read.
Accuracy.  max |pseudo-t - long double| / max |long double| on the device is held to 16 x the float64 restatement's own figure on the same
case, which may not exceed 1e-12 (the rule of the t and TFCE tests); the precondition rss / s0 >= 0.005 is asserted on the inputs first.  With
MET2_GROUP_VSM_PARITY_OUT=<file> the module writes both figures there (profiles/group_vsm_parity.json holds those of an MI355X)."""
import importlib
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import group_numpy as gn                                           # noqa: E402
import group_vsm_numpy as vn                                       # noqa: E402
import tfce_numpy as tn                                            # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
LD = np.longdouble
CEILING = 1e-12
MEASURED = {}
MAX_R, MAX_K, TILE_AXIS, TILE_LINES = 16, 32, 64, 16               # met2_group_vsm_limits (asserted below)
VOXEL_TILE = 256                                                   # met2_group_limits: the t kernel's voxels per block


@pytest.fixture(scope="module")
def group():
    g = importlib.import_module(PKG + ".group")
    assert g.vsm_limits() == {"max_radius": MAX_R, "max_k": MAX_K, "tile_axis": TILE_AXIS, "tile_lines": TILE_LINES}
    assert (g.VSM_MAX_RADIUS, g.VSM_MAX_K) == (MAX_R, MAX_K) and g.limits()["voxel_tile"] == VOXEL_TILE
    yield g
    path = os.environ.get("MET2_GROUP_VSM_PARITY_OUT")
    if path and MEASURED:
        with open(path, "w") as f:
            json.dump({"max_rel_error": MEASURED, "reference": "tests/tools/group_vsm_numpy.py in long double",
                       "measure": "max |pseudo-t - reference| / max |reference|", "bound_factor": 16, "ceiling": CEILING,
                       "device": torch.cuda.get_device_name(0)}, f, indent=1)
            f.write("\n")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def random_taps(rng, radius):
    """positive taps that are neither symmetric nor normalised: the entry takes what it is given"""
    return [rng.random(2 * r + 1) + 0.05 for r in radius]


def check_smooth(group, rng, grid, radius, mask="holes", K=2):
    taps = random_taps(rng, radius)
    maps = rng.standard_normal((K,) + tuple(grid))
    m = {"holes": rng.random(grid) < 0.7, "none": None, "empty": np.zeros(grid, dtype=bool)}[mask] if isinstance(mask, str) else mask
    S, N = group.masked_smooth(maps, m, taps=taps)
    wS, wN = vn.masked_smooth(maps, m, taps)
    assert same(S, wS) and same(N, wN), (grid, radius)
    return S, N


# ---------------------------------------------------------------- met2_masked_smooth

@pytest.mark.parametrize("R", [0, 1, 4, 16])
def test_short_axes_against_every_radius(group, R):
    rng = np.random.default_rng(100 + R)
    for axis in range(3):
        for length in sorted({1, 2, 3, R + 1}):
            grid, radius = [3, 4, 5], [1, 2, 1]
            grid[axis], radius[axis] = length, R
            check_smooth(group, rng, tuple(grid), radius)


def test_anisotropic_radii(group):
    rng = np.random.default_rng(5)
    for radius in sorted(set(itertools.permutations((0, 3, 16)))):
        check_smooth(group, rng, (7, 6, 9), radius)


def test_tile_edges_on_every_axis(group):
    """a pass tiles TILE_AXIS samples along its axis by TILE_LINES lines across it: the lines of the x pass are the ny nz contiguous voxels, of
    the y pass the nz of one x, of the z pass the nx ny rows"""
    rng = np.random.default_rng(6)
    for axis in range(3):
        for length in (TILE_AXIS - 1, TILE_AXIS, TILE_AXIS + 1, 2 * TILE_AXIS + 1):
            grid = [3, 5, 2]
            grid[axis] = length
            check_smooth(group, rng, tuple(grid), (2, 1, 3), K=1)
    for grid in ((2, 3, 5), (2, 4, 4), (2, 1, 17),                 # x: ny nz = 15, 16, 17
                 (2, 3, 15), (2, 3, 16), (2, 3, 17), (2, 3, 33),   # y: nz = 15, 16, 17, and past two tiles
                 (3, 5, 4), (4, 4, 4), (17, 1, 4), (11, 3, 4)):    # z: nx ny = 15, 16, 17, 33
        check_smooth(group, rng, grid, (1, 2, 1), K=1)
    check_smooth(group, rng, (40, 19, 18), (16, 5, 16), K=3)       # several tiles both ways, halos as wide as they get


def test_masks(group):
    rng = np.random.default_rng(7)
    grid = (9, 8, 7)
    check_smooth(group, rng, grid, (2, 2, 2), "holes")
    check_smooth(group, rng, grid, (2, 2, 2), "none")
    corner = np.zeros(grid, dtype=bool)
    corner[-1, -1, -1] = True
    S, N = check_smooth(group, rng, grid, (3, 1, 2), corner)
    assert (N[:5] == 0).all() and N[-1, -1, -1] > 0 and (S[:, :5] == 0).all()
    S, N = check_smooth(group, rng, grid, (3, 1, 2), "empty")
    assert not S.any() and not N.any()


def test_a_map_does_not_depend_on_its_batch(group):
    rng = np.random.default_rng(8)
    grid, radius = (10, 9, 8), (3, 2, 4)
    taps = random_taps(rng, radius)
    mask = rng.random(grid) < 0.7
    maps = rng.standard_normal((MAX_K,) + grid)
    S, N = group.masked_smooth(maps, mask, taps=taps)              # K = 32
    assert same(S, vn.masked_smooth(maps, mask, taps)[0])
    alone, N1 = group.masked_smooth(maps[5], mask, taps=taps)      # K = 1
    assert same(alone, S[5]) and same(N1, N)
    order = rng.permutation(MAX_K)[:7]
    assert same(group.masked_smooth(maps[order], mask, taps=taps)[0], S[order])
    more = group.masked_smooth(np.concatenate([maps, maps[:3]]), mask, taps=taps)[0]      # two calls: 32 + 3
    assert same(more[:MAX_K], S) and same(more[MAX_K:], S[:3])


def test_what_lies_outside_the_mask_is_not_read(group):
    rng = np.random.default_rng(9)
    grid, radius = (8, 7, 9), (2, 3, 1)
    taps = random_taps(rng, radius)
    mask = rng.random(grid) < 0.6
    maps = rng.standard_normal((4,) + grid)
    clean = group.masked_smooth(np.where(mask, maps, 0.0), mask, taps=taps)
    junk = maps.copy()
    junk[:, ~mask] = rng.choice([-0.0, np.inf, -np.inf, np.nan, 1e300], size=(4, int((~mask).sum())))
    dirty = group.masked_smooth(junk, mask, taps=taps)
    assert np.isfinite(dirty[0]).all() and same(dirty[0], clean[0]) and same(dirty[1], clean[1])


def test_smoothing_refusals(group):
    rng = np.random.default_rng(10)
    grid = (4, 4, 4)
    maps = rng.standard_normal((2,) + grid)
    Met2Error = importlib.import_module(PKG + "._lib").Met2Error
    ok = random_taps(rng, (1, 1, 1))
    for bad, code in (([np.ones(2 * MAX_R + 3), ok[1], ok[2]], -2), ([np.array([0.5, 0.0, 0.5]), ok[1], ok[2]], -1),
                      ([ok[0], np.array([0.5, 1.0, np.nan]), ok[2]], -1), ([ok[0], ok[1], np.array([-0.1, 1.0, 0.1])], -1),
                      ([ok[0], ok[1], np.array([np.inf, 1.0, 0.1])], -1)):
        with pytest.raises(Met2Error, match="error %d:" % code):
            group.masked_smooth(maps, None, taps=bad)
    with pytest.raises(ValueError, match="2 R \\+ 1"):
        group.masked_smooth(maps, None, taps=[np.ones(2), ok[1], ok[2]])


# ---------------------------------------------------------------- met2_group_perm_vsm: the cases

GRID = (7, 6, 7)                                                   # 294 voxels: holds 257


def make_case(group, n, r, V, K, seed, grid=GRID, sigma=(1.0, 0.6, 1.4)):
    """a random full-rank design of r columns, the contrast on the first, K distinct permutations, V voxels scattered over the grid"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, r))
    c = np.zeros(r)
    c[0] = 1.0
    W, _ = group.weights(X, c, group.permutation_set(X, c, K, seed=seed))
    assert W.shape == (K, r + 1, n)
    at = np.sort(rng.choice(int(np.prod(grid)), size=V, replace=False)).astype(np.int32)
    Y = rng.standard_normal((n, V)) + 0.7 * X[:, :1]
    Yr, s0 = group.residualise(Y, X, c)
    return Yr, s0, W, grid, at, group.smoothing_taps(sigma)[1]


def run_voxel(group, case, two_sided=False, splits=None):
    """first, kmax and count (accumulated over the launches `splits` cuts the candidates into) against the restatement"""
    Yr, s0, W, grid, at, taps = case
    want0 = vn.perm_vt(Yr, s0, W[:1], grid, at, taps)[0]
    ref = np.abs(want0) if two_sided else want0
    want = vn.perm_vsm(Yr, s0, W, grid, at, "voxel", 1.0, 0.5, 2.0, 6, ref, two_sided, taps)
    _, _, first = group.perm_vsm(Yr, s0, W[:1], grid, at, taps, want_first=True)
    assert same(first, want0)
    count, kmax = None, []
    edges = [0] + list(splits or []) + [W.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        km, count, _ = group.perm_vsm(Yr, s0, W[a:b], grid, at, taps, two_sided=two_sided, ref=ref, count=count)
        kmax.append(km)
    assert same(np.concatenate(kmax), want["kmax"]) and np.array_equal(count, want["count"])
    assert count.min() >= 1                                        # the identity reaches itself
    return want


@pytest.mark.parametrize("n, r, K", [(3, 1, 6), (5, 2, 20), (12, 4, 20), (5, 4, 9), (12, 1, 17)])
def test_voxel_mode_over_subjects_and_columns(group, n, r, K):
    run_voxel(group, make_case(group, n, r, 200, K, seed=20 + n + r), splits=[1, K // 2])


@pytest.mark.parametrize("V", [VOXEL_TILE - 1, VOXEL_TILE, VOXEL_TILE + 1])
def test_voxel_mode_across_the_voxel_tile(group, V):
    run_voxel(group, make_case(group, 5, 2, V, 10, seed=30 + V), splits=[3, 7])


@pytest.mark.parametrize("r, K", [(2, 7), (2, 8), (2, 9), (4, 3), (4, 4), (4, 5), (2, 32), (4, 32)])
def test_voxel_mode_across_the_candidate_groups(group, r, K):
    """the t kernel's groups are 8 candidates up to r = 3 and 4 beyond"""
    run_voxel(group, make_case(group, 12, r, 120, K, seed=40 + 10 * r + K))


def test_two_sided(group):
    case = make_case(group, 8, 2, 150, 24, seed=50)
    one = run_voxel(group, case)
    two = run_voxel(group, case, two_sided=True, splits=[5, 6])
    assert (one["s"] < 0).any() and (two["s"] >= 0).all() and (two["kmax"] >= one["kmax"]).all()


def test_a_candidate_does_not_depend_on_its_batch(group):
    Yr, s0, W, grid, at, taps = make_case(group, 8, 2, 180, MAX_K, seed=51)
    km = group.perm_vsm(Yr, s0, W, grid, at, taps)[0]
    order = np.random.default_rng(1).permutation(MAX_K)[:11]
    assert same(group.perm_vsm(Yr, s0, W[order], grid, at, taps)[0], km[order])
    assert same(group.perm_vsm(Yr, s0, W[9:10], grid, at, taps)[0], km[9:10])


def test_unit_taps_give_perm_stats_to_the_bit(group):
    Yr, s0, W, grid, at, _ = make_case(group, 8, 3, VOXEL_TILE + 1, 20, seed=52)
    s0 = s0.copy()
    s0[17] = 0.0                                                   # rss <= 0 there: t = 0 for both
    one = [np.ones(1)] * 3
    for two in (False, True):
        _, _, t0 = group.perm_stats(Yr, s0, W[:1], want_first=True)
        ref = np.abs(t0) if two else t0
        a = group.perm_stats(Yr, s0, W, two_sided=two, t_ref=ref, want_first=True)
        b = group.perm_vsm(Yr, s0, W, grid, at, one, two_sided=two, ref=ref, want_first=True)
        assert same(a[0], b[0]) and np.array_equal(a[1], b[1]) and same(a[2], b[2]) and b[2][17] == 0.0


def test_a_voxel_without_residual_variance(group):
    """rss <= 0 at a voxel gives rho = 0 there; its pseudo-t lives on its neighbours' variance, and theirs takes a zero from it"""
    Yr, s0, W, grid, at, taps = make_case(group, 8, 2, 200, 12, seed=53)
    s0 = s0.copy()
    s0[[40, 41, 150]] = 0.0
    want = run_voxel(group, (Yr, s0, W, grid, at, taps))
    assert np.isfinite(want["s"]).all() and (want["s"][:, 40] != 0).any()


def test_a_value_that_is_not_a_number(group):
    Yr, s0, W, grid, at, taps = make_case(group, 8, 2, 200, 12, seed=54)
    Yr, s0 = Yr.copy(), s0.copy()
    j = 77
    Yr[2, j], s0[j] = np.nan, np.nan
    want = vn.perm_vsm(Yr, s0, W, grid, at, "voxel", 1.0, 0.5, 2.0, 6, None, False, taps)
    assert np.isnan(want["s"][:, j]).all() and np.isfinite(np.delete(want["s"], j, axis=1)).all() and np.isfinite(want["kmax"]).all()
    ref = np.where(np.isnan(want["s"][0]), 0.0, want["s"][0])
    wc = (want["s"] >= ref[None, :]).sum(axis=0)
    km, count, first = group.perm_vsm(Yr, s0, W, grid, at, taps, ref=ref, want_first=True)
    rest = np.delete(np.arange(at.size), j)
    assert np.isnan(first[j]) and same(first[rest], want["s"][0][rest])        # every neighbour equals the restatement
    assert same(km, want["kmax"])                                  # the maximum passes over it
    assert np.array_equal(count, wc) and count[j] == 0             # and it reaches no reference
    # the lane that holds it must not hide the maxima that pass through it in the wave's exchange: the same with the largest values around it
    big = Yr.copy()
    big[:, j - 33:j + 33] += 2.0 * W[0, 0][:, None]               # along the identity's effect row: its pseudo-t peaks there
    big[2, j] = np.nan
    sb = np.sum(big * big, axis=0)
    wb = vn.perm_vsm(big, sb, W, grid, at, "voxel", 1.0, 0.5, 2.0, 6, None, False, taps)
    assert np.isfinite(wb["kmax"]).all() and same(group.perm_vsm(big, sb, W, grid, at, taps)[0], wb["kmax"])


def test_group_entry_refusals_leave_the_outputs_untouched(group):
    Met2Error = importlib.import_module(PKG + "._lib").Met2Error
    Yr, s0, W, grid, at, taps = make_case(group, 6, 2, 60, 4, seed=55)
    dev = torch.device("cuda", 0)
    put = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    Yt, st, at_t = put(Yr), put(s0), put(at)
    ref = put(np.zeros(at.size))
    radius = tuple((t.size - 1) // 2 for t in taps)

    def refused(code, W_=W, two=False, mode="voxel", radius_=radius, taps_=taps, at_=at_t, dh=1.0):
        first = torch.full((at.size,), -7.0, dtype=torch.float64, device=dev)
        kmax = torch.full((W_.shape[0],), -7.0, dtype=torch.float64, device=dev)
        count = torch.full((at.size,), 3, dtype=torch.int32, device=dev)
        with pytest.raises(Met2Error, match="error %d:" % code):
            group._launch_vsm(dev, Yt, st, 2, put(W_), two, grid, at_, mode, dh, 0.5, 2.0, 6, radius_, taps_, ref, first, kmax, count, None)
        torch.cuda.synchronize()
        assert (first == -7.0).all() and (kmax == -7.0).all() and (count == 3).all()

    wide = [np.ones(2 * MAX_R + 3) / 35.0, taps[1], taps[2]]
    refused(-2, radius_=(MAX_R + 1, radius[1], radius[2]), taps_=wide)
    refused(-2, W_=np.concatenate([W] * 9)[:MAX_K + 1])
    refused(-1, radius_=(-1, radius[1], radius[2]))
    for bad in (np.nan, np.inf, -0.25):
        t = [x.copy() for x in taps]
        t[1][0] = bad
        refused(-1, taps_=t)
    t = [x.copy() for x in taps]
    t[2][radius[2]] = 0.0                                          # the centre tap
    refused(-1, taps_=t)
    refused(-1, two=True, mode="tfce")
    refused(-1, two=True, mode="extent")
    refused(-1, mode="tfce", dh=0.0)
    swapped = at.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    for mode in ("voxel", "tfce", "extent"):                       # late: the device finds it, and nothing has been written
        refused(-1, at_=put(swapped), mode=mode)
    beyond = at.copy()
    beyond[-1] = int(np.prod(grid))
    refused(-1, at_=put(beyond))


# ---------------------------------------------------------------- the spatial modes

@pytest.mark.parametrize("mode, connectivity", [("tfce", 6), ("tfce", 26), ("extent", 26), ("extent", 6)])
def test_spatial_modes_on_the_pseudo_t(group, mode, connectivity):
    Yr, s0, W, grid, at, taps = make_case(group, 8, 2, 230, 12, seed=60, sigma=1.0)
    t0 = vn.perm_vt(Yr, s0, W[:1], grid, at, taps)[0]
    dh = t0.max() / 100.0 if mode == "tfce" else 1.5
    obs = vn.perm_vsm(Yr, s0, W[:1], grid, at, mode, dh, 0.5, 2.0, connectivity, None, False, taps)["s"][0]
    want = vn.perm_vsm(Yr, s0, W, grid, at, mode, dh, 0.5, 2.0, connectivity, obs, False, taps)
    assert obs.max() > 0 and (obs == 0).any()
    _, _, first = group.perm_vsm(Yr, s0, W[:1], grid, at, taps, mode=mode, dh=dh, connectivity=connectivity, want_first=True)
    assert same(first, obs)
    km1, count, _ = group.perm_vsm(Yr, s0, W[:5], grid, at, taps, mode=mode, dh=dh, connectivity=connectivity, ref=obs)
    km2, count, _ = group.perm_vsm(Yr, s0, W[5:], grid, at, taps, mode=mode, dh=dh, connectivity=connectivity, ref=obs, count=count)
    assert same(np.concatenate([km1, km2]), want["kmax"]) and np.array_equal(count, want["count"])


# ---------------------------------------------------------------- the filter against the host

def test_filter_equals_the_host_run_of_the_planted_case(group):
    filters = importlib.import_module(PKG + ".filters")
    Y, X, c, grid, at, block, near, plain, vsm, both = vn.planted_host(group)
    vols = Y.reshape((Y.shape[0],) + tuple(grid))
    dev = filters.group_stats_filter(vols, X, c, variance_smoothing=vn.PLANTED_SIGMA, tfce=True, n_perm=64, seed=0, exchange="flip")
    assert dev["mask"].all() and dev["variance_smoothing"] == both["variance_smoothing"]
    for key, want in both.items():
        if key == "variance_smoothing":
            continue
        got = dev[key]
        if isinstance(want, np.ndarray):
            assert np.array_equal(np.asarray(got).reshape(want.shape), want), key
        else:
            assert got == want, key
    hits = lambda res, key: int(((np.asarray(res[key]).reshape(-1) <= 0.05) & block).sum())
    assert hits(dev, "p_fwe") == hits(both, "p_fwe") and hits(dev, "p_tfce_fwe") == hits(both, "p_tfce_fwe")
    assert hits(dev, "p_fwe") >= 10 * hits(plain, "p_fwe")
    voxel_only = filters.group_stats_filter(vols, X, c, variance_smoothing=vn.PLANTED_SIGMA, n_perm=64, seed=0, exchange="flip", two_sided=True)
    assert np.array_equal(voxel_only["tstat"].reshape(-1), vsm["tstat"])


# ---------------------------------------------------------------- accuracy against long double

def test_accuracy_against_long_double(group):
    Yr, s0, W, grid, at, taps = make_case(group, 12, 2, VOXEL_TILE + 1, 8, seed=70)
    ratio = gn.perm_t(Yr, s0, W, False, LD)[1]
    assert float(ratio.min()) >= 0.005, "the project's precondition rss / s0 >= 0.005 does not hold on this case"
    ref = vn.perm_vt(Yr, s0, W, grid, at, taps, dtype=LD)
    rel = lambda got: float(np.abs(np.asarray(got, dtype=LD) - ref).max() / np.abs(ref).max())
    host = rel(vn.perm_vt(Yr, s0, W, grid, at, taps))
    dev = rel(np.stack([group.perm_vsm(Yr, s0, W[k:k + 1], grid, at, taps, want_first=True)[2] for k in range(W.shape[0])]))
    MEASURED.update(device=dev, float64_restatement=host)
    print("pseudo-t against long double: device %.3g, float64 restatement %.3g" % (dev, host))
    bound = min(16.0 * host, CEILING)
    assert 0.0 < host and dev <= bound, (dev, host, bound)
