"""The cluster mass without a device: the numpy restatement of MET2_TFCE_MODE_MASS (tests/tools/cluster_mass_numpy.py: scipy.ndimage.label and
an int64 np.add.at) against hand-worked cases and against brute force that shares nothing with it (flood fill, Python integers, the
quantisation in exact rationals), and group.randomise(cluster_mass_threshold=...) with the float64 restatements as stand-ins -- the loops
whose bits the device is held to in tests/test_gpu_cluster_mass.py.
Bounds.  Hand-worked cases and the brute force: equal.  p-values: ratios of integers, equal.  The fixed point against the exact sum: a
member's q differs from t 2^24 by at most 1/2, so the integer total differs from the exact sum by at most e / 2 units of 2^-24 = e 2^-25
for a component of e voxels, and the conversion to double adds one rounding, at most half an ulp of the result: the test holds
|out - long double sum| to e 2^-25 + ulp(out) / 2 (+ the long double sum's own error, 64-bit mantissa: below 1e-3 of the bound) and prints
the worst ratio of the first term's share (measured: 0.8181 on these random maps; 0.9995 on the planted case's t maps).
Planted effect (tfce_numpy.planted_case(): n = 12 one-sample, 400 of the 4 096 sign flips, seed 0, threshold 2.5, connectivity 26).
Measured here with the restatement: p_mass_fwe <= 0.05 in 128 of the 144 block voxels, 1 voxel in the one-voxel shell, none beyond it;
mass_crit 18.76 (the extent finds the same 128: at this threshold the block is one component either way).  The test asks for at least half
the block and nothing farther than one voxel from it, as the TFCE host test does."""
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import cluster_mass_numpy as cm                                    # noqa: E402
import group_f_numpy as gf                                         # noqa: E402
import group_numpy as gn                                           # noqa: E402
import group_vsm_numpy as gv                                       # noqa: E402
import tfce_numpy as tn                                            # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"
U = 2.0 ** -24                                                     # one unit of the fixed point


@pytest.fixture(scope="module")
def group():
    return importlib.import_module(PKG + ".group")


def line(values):
    return np.asarray(values, dtype=np.float64).reshape(1, 1, -1)


# ---------------------------------------------------------------- hand-worked cases

def test_two_components_of_equal_size_and_different_height_by_hand():
    t = line([3.0, 3.5, 0.0, 6.0, 7.25, 1.0])
    assert np.array_equal(cm.transform(t, 2.0, connectivity=6).ravel(), [6.5, 6.5, 0.0, 13.25, 13.25, 0.0])
    ext = tn.transform(t, None, "extent", 2.0, connectivity=6)[0].ravel()
    assert np.array_equal(ext, [2, 2, 0, 2, 2, 0])                 # the extent cannot tell them apart; the mass does
    # a corner contact joins two voxels under 26 only
    t = np.zeros((2, 2, 2))
    t[0, 0, 0], t[1, 1, 1] = 2.5, 4.0
    assert np.array_equal(cm.transform(t, 2.0, connectivity=26)[[0, 1], [0, 1], [0, 1]], [6.5, 6.5])
    assert np.array_equal(cm.transform(t, 2.0, connectivity=18)[[0, 1], [0, 1], [0, 1]], [2.5, 4.0])


def test_threshold_and_one_ulp_below_it():
    h = 3 * 0.3
    t = line([h, np.nextafter(h, 0), 5.0])
    out = cm.transform(t, h, connectivity=6).ravel()
    assert out[0] == float(cm.quantise(h)) * U and out[1] == 0.0 and out[2] == 5.0      # the gap keeps the two members apart
    assert abs(out[0] - h) <= U / 2 and np.array_equal(tn.transform(t, None, "extent", h)[0].ravel(), [1, 0, 1])


def test_a_tie_goes_to_even_and_the_sum_is_of_the_quantised_values():
    a, b = (2.0 ** 24 + 0.5) * U, (2.0 ** 24 + 1.5) * U             # q + 1/2 with q even and with q odd
    assert cm.quantise(a) == 2 ** 24 and cm.quantise(b) == 2 ** 24 + 2
    assert cm._q_exact(a) == 2 ** 24 and cm._q_exact(b) == 2 ** 24 + 2
    out = cm.transform(line([a, b]), 1.0, connectivity=6).ravel()
    assert np.array_equal(out, [2.0 + 2 * U] * 2)                  # here the two roundings cancel: the raw sum is 2 + 2 u as well
    three = cm.transform(line([a, a, b]), 1.0, connectivity=6).ravel()             # the raw sum is 3 + 2.5 u, that of the integers 3 + 2 u
    assert np.array_equal(three, [3.0 + 2 * U] * 3) and (a + a) + b != three[0]


def test_saturation_above_the_cap_and_at_infinity():
    t = line([cm.T_CAP * 2, np.inf, cm.T_CAP, 1.0, 0.0, np.nextafter(cm.T_CAP, 0)])
    out = cm.transform(t, 0.5, connectivity=6).ravel()
    assert np.array_equal(out[:4], [3 * cm.T_CAP + 1.0] * 4) and out[4] == 0.0 and out[5] == cm.T_CAP     # one ulp below the cap rounds up to it
    assert cm.quantise(np.inf) == 2 ** 38 and cm.MAX_G * 2 ** 38 == 2 ** 62        # the largest sum the definition admits fits in int64


def test_what_joins_no_component():
    t = line([3.0, np.nan, 3.0, -np.inf, 3.0, -0.0, 3.0, 9.0, 3.0])
    mask = line([1, 1, 1, 1, 1, 1, 1, 0, 1]).astype(np.uint8)
    out = cm.transform(t, 1.0, mask, connectivity=26).ravel()
    assert np.array_equal(out, [3.0, 0.0, 3.0, 0.0, 3.0, 0.0, 3.0, 0.0, 3.0]) and not np.signbit(out).any()
    assert (cm.transform(line([np.nan, -1.0, 0.5]), 1.0) == 0).all()                # nothing above the threshold


# ---------------------------------------------------------------- the restatement against brute force and the bound

@pytest.fixture(scope="module")
def brute_map():
    rng = np.random.default_rng(7)
    t = rng.standard_normal((5, 4, 3)) * 1.5
    t[0, 0, 0], t[1, 1, 1], t[2, 2, 2], t[4, 3, 2], t[3, 0, 1] = 0.5, np.nextafter(0.5, 0), np.nan, -0.0, np.inf
    mask = rng.random((5, 4, 3)) < 0.8
    mask[3, 0, 1] = True
    return t, mask


@pytest.mark.parametrize("connectivity", [6, 18, 26])
def test_against_flood_fill_and_python_integers(brute_map, connectivity):
    t, mask = brute_map
    for m in (None, mask):
        got = cm.transform(t, 0.5, m, connectivity)
        assert np.array_equal(got, cm.flood_mass(t, 0.5, m, connectivity))
        assert np.array_equal(got > 0, tn.transform(t, m, "extent", 0.5, connectivity=connectivity)[0] > 0)   # membership is the extent's
    assert cm.transform(t, 0.5, mask, connectivity)[3, 0, 1] >= cm.T_CAP


def test_bound_against_the_long_double_sum():
    rng = np.random.default_rng(11)
    worst = 0.0
    for scale, h, conn in ((1.5, 0.5, 26), (1.5, 0.1, 6), (40.0, 3.0, 18), (1e-3, 1e-4, 26)):
        t = rng.standard_normal((12, 11, 10)) * scale
        out = cm.transform(t, h, None, conn)
        exact, e = cm.exact_sum(t, h, None, conn)
        err = np.abs(out.astype(np.longdouble) - exact).astype(np.float64)
        bound = e * 2.0 ** -25 + np.spacing(out) / 2
        assert (e > 50).any() and (err <= bound * (1 + 1e-3)).all()
        worst = max(worst, float((err[e > 0] / (e[e > 0] * 2.0 ** -25)).max()))
    print("worst |out - exact| / (e 2^-25): %.4f" % worst)


# ---------------------------------------------------------------- randomise

@pytest.fixture(scope="module")
def small(group):
    """tests/test_tfce_host.py's small case through randomise without and with the mass: n = 8, 64 sign flips, grid 6 x 5 x 4, 100 voxels"""
    rng = np.random.default_rng(12)
    grid = (6, 5, 4)
    at = np.sort(rng.choice(120, 100, replace=False))
    Y = rng.standard_normal((8, 100)) + 0.4
    Y[:, 50] = 0.0                                                 # a voxel that is left out of the launches
    X, c = gn.one_sample_design(8)
    kw = dict(n_perm=64, seed=2, exchange="flip", batch_stat=gn.batch_stat)
    sp = dict(grid=grid, at=at, batch_spatial=cm.batch_spatial)
    before = group.randomise(Y, X, c, tfce=True, cluster_threshold=1.5, **sp, **kw)
    mass = group.randomise(Y, X, c, tfce=True, cluster_threshold=1.5, cluster_mass_threshold=1.5, **sp, **kw)
    alone = group.randomise(Y, X, c, cluster_mass_threshold=1.5, **sp, **kw)
    return Y, X, c, grid, at, kw, sp, before, mass, alone


MASS_KEYS = ("cluster_mass", "p_mass_uncorrected", "p_mass_fwe", "mass_count", "mass_max_dist", "mass_crit", "cluster_mass_threshold")


def test_nothing_else_changes_when_the_option_is_added(group, small):
    Y, X, c, grid, at, kw, sp, before, mass, alone = small
    assert set(mass) - set(before) == set(MASS_KEYS)
    for key, val in before.items():
        assert np.array_equal(val, mass[key]), key
    plain = group.randomise(Y, X, c, **kw)
    assert set(alone) - set(plain) == set(MASS_KEYS) | {"cluster_connectivity"}
    for key, val in plain.items():
        assert np.array_equal(val, alone[key]), key
    for key in MASS_KEYS:
        assert np.array_equal(alone[key], mass[key]), key


def test_identity_is_counted_and_p_is_a_ratio(small):
    Y, X, c, grid, at, kw, sp, before, out, _ = small
    P = out["n_perm"]
    md, stat = out["mass_max_dist"], out["cluster_mass"]
    assert P == 64 and md.shape == (P,) and md[0] == stat.max() and out["cluster_mass_threshold"] == 1.5 and out["cluster_connectivity"] == 26
    assert out["p_mass_uncorrected"].min() >= 1.0 / P and out["p_mass_fwe"].min() >= 1.0 / P and (out["p_mass_fwe"] >= out["p_mass_uncorrected"]).all()
    assert np.array_equal(out["p_mass_uncorrected"], out["mass_count"] / float(P))
    assert np.array_equal(out["p_mass_fwe"], (md[:, None] >= stat[None, :]).sum(axis=0) / float(P))
    assert out["mass_crit"] == np.quantile(md, 0.95)
    outside = stat == 0
    assert outside.any() and (out["p_mass_fwe"][outside] == 1.0).all() and (out["mass_count"][outside] == P).all()
    assert stat[50] == 0 and out["p_mass_fwe"][50] == 1.0 and out["mass_count"][50] == P          # the left-out voxel
    maps, mask = tn.dense(out["tstat"][None, :], grid, at)
    mask.reshape(-1)[at[50]] = 0
    assert np.array_equal(stat, cm.transform(maps[0], 1.5, mask, 26).reshape(-1)[at])
    assert np.array_equal(stat > 0, out["cluster_extent"] > 0) and (stat[stat > 0] >= 1.5 * out["cluster_extent"][stat > 0] - 1e-6).all()


def test_a_cropped_grid_changes_nothing(group, small):
    Y, X, c, grid, at, kw, sp, before, out, _ = small
    x, y, z = np.unravel_index(at, grid)
    big = (9, 8, 7)
    again = group.randomise(Y, X, c, cluster_mass_threshold=1.5, grid=big, at=np.ravel_multi_index((x + 2, y + 1, z + 3), big),
                            batch_spatial=cm.batch_spatial, **kw)
    for key in MASS_KEYS:
        assert np.array_equal(out[key], again[key]), key


def test_on_f_and_on_the_pseudo_t(group):
    rng = np.random.default_rng(21)
    grid = (5, 4, 3)
    at = np.sort(rng.choice(60, 50, replace=False))
    X, fc = gf.three_group_design((3, 3, 3), covariate=False)
    Y = rng.standard_normal((9, 50))
    Y[3:6, :20] += 2.0
    kw = dict(n_perm=40, seed=1, grid=grid, at=at)
    f = group.randomise(Y, X, f_contrast=fc, batch_stat=gf.batch_stat, batch_spatial=cm.batch_spatial_f, cluster_mass_threshold=3.0,
                        cluster_connectivity=18, **kw)
    maps, mask = tn.dense(f["fstat"][None, :], grid, at)
    assert np.array_equal(f["cluster_mass"], cm.transform(maps[0], 3.0, mask, 18).reshape(-1)[at]) and (f["cluster_mass"] > 0).any()
    assert f["mass_max_dist"][0] == f["cluster_mass"].max() and np.array_equal(f["p_mass_uncorrected"], f["mass_count"] / float(f["n_perm"]))
    f0 = group.randomise(Y, X, f_contrast=fc, batch_stat=gf.batch_stat, **{k: kw[k] for k in ("n_perm", "seed")})
    for key, val in f0.items():
        assert np.array_equal(val, f[key]), key
    X1, c = gn.one_sample_design(9)
    v = group.randomise(Y + 0.5, X1, c, exchange="flip", batch_stat=gn.batch_stat, batch_spatial=cm.batch_spatial_vsm, variance_smoothing=1.0,
                        cluster_mass_threshold=1.0, **kw)
    maps, mask = tn.dense(v["tstat"][None, :], grid, at)
    assert np.array_equal(v["cluster_mass"], cm.transform(maps[0], 1.0, mask, 26).reshape(-1)[at]) and (v["cluster_mass"] > 0).any()
    assert v["mass_max_dist"][0] == v["cluster_mass"].max() and np.array_equal(v["p_mass_uncorrected"], v["mass_count"] / float(v["n_perm"]))
    v0 = group.randomise(Y + 0.5, X1, c, exchange="flip", batch_stat=gn.batch_stat, batch_spatial=cm.batch_spatial_vsm, variance_smoothing=1.0, **kw)
    for key, val in v0.items():
        assert np.array_equal(val, v[key]), key


def test_refusals(group, small):
    Y, X, c, grid, at, kw, sp, *_ = small
    with pytest.raises(ValueError, match="one-sided"):
        group.randomise(Y, X, c, cluster_mass_threshold=2.0, two_sided=True, **sp, **kw)
    with pytest.raises(ValueError, match="one-sided"):
        group.randomise(Y, X, c, cluster_mass_threshold=2.0, two_sided=True, variance_smoothing=1.0, grid=grid, at=at,
                        batch_spatial=cm.batch_spatial_vsm, **kw)
    with pytest.raises(ValueError, match="grid"):
        group.randomise(Y, X, c, cluster_mass_threshold=2.0, batch_spatial=cm.batch_spatial, **kw)
    with pytest.raises(ValueError, match="grid"):
        group.randomise(Y, X, c, cluster_mass_threshold=2.0, grid=grid, batch_spatial=cm.batch_spatial, **kw)
    with pytest.raises(ValueError, match="batch_spatial"):
        group.randomise(Y, X, c, cluster_mass_threshold=2.0, grid=grid, at=at, **kw)
    with pytest.raises(ValueError, match="cluster_mass_threshold"):
        group.randomise(Y, X, c, cluster_mass_threshold=-1.0, **sp, **kw)
    with pytest.raises(ValueError, match="cluster_mass_threshold"):
        group.randomise(Y, X, c, cluster_mass_threshold=float("nan"), **sp, **kw)
    with pytest.raises(ValueError, match="connectivity"):
        group.randomise(Y, X, c, cluster_mass_threshold=2.0, cluster_connectivity=8, **sp, **kw)
    assert group.MODES["mass"] == 3 and group.VSM_MODES == dict(group.MODES, voxel=2)


# ---------------------------------------------------------------- the planted effect

def test_planted_block_is_found_by_the_mass_and_nothing_far_from_it(group):
    Y, X, c, grid, at, block, near = tn.planted_case()
    out = group.randomise(Y, X, c, n_perm=400, seed=0, exchange="flip", batch_stat=gn.batch_stat, batch_spatial=cm.batch_spatial,
                          cluster_mass_threshold=2.5, cluster_connectivity=26, grid=grid, at=at)
    found = out["p_mass_fwe"] <= 0.05
    print("mass: %d of %d block voxels, %d in the shell, %d beyond; mass_crit %.4f; largest observed mass %.4f"
          % (found[block].sum(), block.sum(), found[near & ~block].sum(), found[~near].sum(), out["mass_crit"], out["cluster_mass"].max()))
    assert out["n_perm"] == 400 and not out["exhaustive"] and block.sum() == 144
    assert found[block].sum() >= 72 and not found[~near].any()
