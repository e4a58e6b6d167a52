"""met2_group_perm_fstats and met2_group_perm_ftfce on the device (include/met2_hip.h states the contract) against their numpy restatement
(tests/tools/group_f_numpy.py), and group_stats_filter(f_contrast=...) end to end against the host run of tests/test_group_f_host.py's
planted three-group case.
Equality.  The header fixes the order of every sum and forbids fused products, so numpy reproduces the entry in float64: the device's F, kmax
and count must EQUAL the float64 restatement's, bit for bit, on every case -- which also says that the bits depend on nothing but W[k],
Y[:, v], s0[v], s and scale.  The same is tested from the device alone: a batch reordered, the voxels reordered, K = 1 launches against one
launch of max_k, a set split over three launches, all weights negated, and the identity's own F fed back as f_ref.
Accuracy.  max |F - long double| / max |long double| <= 16 x the largest such figure measured on an MI355X over these very cases
(profiles/group_f_parity.json, beside it the float64 restatement's own figure), which may not exceed 1e-12.  With
MET2_GROUP_F_PARITY_OUT=<file> the module writes what it measured there.  s = 1: |F - t^2| of the existing met2_group_perm_stats, relative to
the largest t^2, within the sum of the two entries' bounds.
Inputs: seeded normal data plus a mean of 0.3, residualised against the case's nuisance; designs of a constant and r - 1 seeded covariates,
the contrast matrix the first s columns of the identity, sign flips (row 0 the identity; K below 2^n, since the all-flipped pattern gives
the identity's F).  Before any device call every case asserts on the long-double restatement that rss / s0 >= 0.005 for every (k, v) -- the
rounding error of F grows as 1 / (rss / s0) -- and that no candidate other than the identity has an F within 1e-10 max F of the voxel's
observed F, so no comparison F >= f_ref hangs on a rounding and no case is left out of any comparison.  The seeds were chosen on the host
so that both hold.
Shapes (CASES): n in {3, 5, 12, max_n}, r in {1, 2, 4, 5, max_r} (KB = 8 up to r = 4, 4 beyond), s in {1, 2, r}, V in {1, 63, 64, 65,
tile - 1, tile, tile + 1, 4 096}, K in {1, KB - 1, KB, KB + 1, 32, max_k}; f_ref and f_first each NULL and given.
Spatial: met2_group_perm_ftfce equals met2_tfce applied to the device's own F maps and the restatement, to the bit, at E = 0.5, H = 2 with
connectivity 6 and 26 in TFCE and extent mode, on a 12 x 10 x 8 grid with a mask, K in {1, 5, 32}; a row does not depend on K or its mates."""
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
import group_f_numpy as gf                                         # noqa: E402
import tfce_numpy as tn                                            # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
CEILING = 1e-12
MEASURED = {"F": 0.0, "F_float64_restatement": 0.0}
INVALID, UNSUPPORTED = -1, -2                                      # MET2_E_INVALID, MET2_E_UNSUPPORTED
LD = np.longdouble
MAX_N, MAX_R, MAX_K, TILE, TFCE_MAX_K = 128, 8, 256, 256, 32       # met2_group_limits, met2_tfce_limits (asserted below)
KB = lambda r: 8 if r <= 4 else 4                                  # the F kernel's candidates per group

# name -> (n, r, s, V, K, seed)
CASES = {
    "n3_r1_s1_v1_k1": (3, 1, 1, 1, 1, 1),
    "n3_r2_s2_v1_k7": (3, 2, 2, 1, 7, 43),
    "n5_r1_s1_tile_plus_1_k8": (5, 1, 1, TILE + 1, 8, 2),
    "n5_r2_s1_v63_k9": (5, 2, 1, 63, 9, 2),
    "n5_r4_s4_v1_k9": (5, 4, 4, 1, 9, 8),
    "n12_r4_s2_v65_k32": (12, 4, 2, 65, 32, 1),
    "n12_r4_s4_v63_k8": (12, 4, 4, 63, 8, 1),
    "n12_r5_s2_v4096_k5": (12, 5, 2, 4096, 5, 1),
    "n12_r5_s5_tile_minus_1_k3": (12, 5, 5, TILE - 1, 3, 1),
    "n12_r5_s1_tile_k4": (12, 5, 1, TILE, 4, 1),
    "n12_rmax_s2_v64_k32": (12, MAX_R, 2, 64, 32, 1),
    "nmax_rmax_smax_tile_minus_1_kmax": (MAX_N, MAX_R, MAX_R, TILE - 1, MAX_K, 1),
    "nmax_r2_s2_tile_k9": (MAX_N, 2, 2, TILE, 9, 1),
    "n12_r2_s2_v4096_kmax": (12, 2, 2, 4096, MAX_K, 1),
    "n12_r1_s1_v64_k1": (12, 1, 1, 64, 1, 1),
    "n12_r2_s1_v65_k7": (12, 2, 1, 65, 7, 1),
}


def _json(name):
    path = os.path.join(ROOT, "profiles", name)
    assert os.path.exists(path), "%s is missing: it holds the measured figures the bounds derive from" % path
    return json.load(open(path))


def rel_err(got, want):
    want = np.asarray(want, dtype=LD)
    return float(np.abs(np.asarray(got, dtype=LD) - want).max() / np.abs(want).max())


def bound(quantity="F", profile="group_f_parity.json"):
    b = 16.0 * float(_json(profile)["max_rel_error"][quantity])
    assert 0.0 < b <= CEILING, "the measured error of %s puts the bound at %g: above %g it is a defect, not rounding" % (quantity, b, CEILING)
    return b


def held(got, want, f64=None):
    """records max |got - want| / max |want|, prints it, and holds it to the bound"""
    err = rel_err(got, want)
    MEASURED["F"] = max(MEASURED["F"], err)
    if f64 is not None:
        MEASURED["F_float64_restatement"] = max(MEASURED["F_float64_restatement"], rel_err(f64, want))
    print("F: relative error %.3g" % err)
    b = bound()
    assert err <= b, (err, b)


@pytest.fixture(scope="module")
def group():
    g = importlib.import_module(PKG + ".group")
    assert g.limits() == {"max_n": MAX_N, "max_r": MAX_R, "max_k": MAX_K, "voxel_tile": TILE} and g.tfce_limits()["max_k"] == TFCE_MAX_K
    yield g
    path = os.environ.get("MET2_GROUP_F_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"max_rel_error": MEASURED, "reference": "tests/tools/group_f_numpy.py in long double",
                       "measure": "max |error| / max |reference| per case", "bound_factor": 16, "ceiling": CEILING,
                       "device": torch.cuda.get_device_name(0)}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib").lib()


def make_inputs(group, n, r, s, V, K, seed):
    """(Yr [n, V], s0 [V], W [K, r, n], scale) of a constant and r - 1 covariates, the contrast matrix the first s columns of the identity,
    under K sign flips, the identity first"""
    rng = np.random.default_rng([seed, n, r, s, V, K])
    X = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, r - 1))], axis=1)
    Cm = np.eye(r)[:, :s]
    perms = group.permutation_set(X, Cm, K, seed, "flip")
    assert len(perms.index) == K and K < 2 ** n, "the design has no %d arrangements short of the exhaustive set" % K
    W, s_, dof = group.weights_f(X, Cm, perms)
    assert s_ == s and W.shape == (K, r, n)
    Yr, s0 = group.residualise(rng.standard_normal((n, V)) + 0.3, X, Cm)
    return Yr, s0, W, float(dof) / s


def preconditions(ld):
    """on the long-double restatement: no rss near 0, no candidate's F near the observed one"""
    assert ld["ratio"].min() >= 0.005, "rss / s0 falls to %g" % ld["ratio"].min()
    if ld["F"].shape[0] > 1:
        gap = np.abs(ld["F"][1:] - ld["F"][0][None, :]).min()
        assert gap > 1e-10 * np.abs(ld["F"]).max(), "a candidate's F lies within %g of the observed one" % gap


_CACHE = {}


def host_case(group, name):
    """the inputs of a case and its restatements (long double and float64), with the preconditions asserted: no device call"""
    n, r, s, V, K, seed = CASES[name]
    Y, s0, W, scale = make_inputs(group, n, r, s, V, K, seed)
    ld = gf.perm_fstats(Y, s0, W, s, scale, None, LD)
    f64 = gf.perm_fstats(Y, s0, W, s, scale, None, np.float64)
    preconditions(ld)
    return dict(Y=Y, s0=s0, W=W, s=s, scale=scale, ld=ld, f64=f64)


def case(group, name):
    """host_case plus the device's own table of F, got with K = 1 launches and f_first; computed once and shared"""
    if name not in _CACHE:
        cs = host_case(group, name)
        cs["table"] = device_table(group, cs["Y"], cs["s0"], cs["W"], cs["s"], cs["scale"])
        _CACHE[name] = cs
    return _CACHE[name]


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda").to(dtype).contiguous()


def device_table(group, Y, s0, W, s, scale):
    """F [K, V] from the device: one launch of K = 1 per candidate, f_first (no f_ref, no count); the K kmax must be the rows' maxima"""
    Yt, st, Wt = dev(Y), dev(s0), dev(W)
    K, V = W.shape[0], Y.shape[1]
    table = torch.empty((K, V), dtype=torch.float64, device="cuda")
    kmax = torch.empty(K, dtype=torch.float64, device="cuda")
    d = torch.device("cuda", 0)
    for k in range(K):
        group._launch_f(d, Yt, st, Wt[k:k + 1], s, scale, None, table[k], kmax[k:k + 1], None)
    table = table.cpu().numpy()
    assert np.array_equal(kmax.cpu().numpy(), table.max(axis=1))
    return table


# ---------------------------------------------------------------- parity and equality, per case

@pytest.mark.parametrize("name", sorted(CASES))
def test_f_is_the_float64_restatement_to_the_bit_and_long_double_to_the_bound(group, name):
    cs = case(group, name)
    assert np.array_equal(cs["table"], cs["f64"]["F"]), "the device's F differs from numpy's float64 loop in the entry's order"
    held(cs["table"], cs["ld"]["F"], cs["f64"]["F"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_kmax_count_and_f_first_of_one_launch(group, name):
    cs = case(group, name)
    Y, s0, W, s, scale, table = cs["Y"], cs["s0"], cs["W"], cs["s"], cs["scale"], cs["table"]
    f_ref = table[0].copy()                                        # the observed statistic: the identity is candidate 0
    kmax, count, first = group.perm_fstats(Y, s0, W, s, scale, f_ref=f_ref, want_first=True)
    want = gf.perm_fstats(Y, s0, W, s, scale, f_ref, np.float64)
    assert count.dtype == np.uint32 and np.array_equal(count, want["count"])
    assert np.array_equal(kmax, table.max(axis=1)) and np.array_equal(kmax, want["kmax"])
    assert np.array_equal(first, table[0])
    # the long-double restatement counts the same candidates: none but the identity is close to the observed F
    assert np.array_equal(count, 1 + (cs["ld"]["F"][1:] >= f_ref[None, :]).sum(axis=0))
    assert (count >= 1).all()
    # f_ref NULL: no count; f_first NULL: the same kmax
    kmax2, none, none2 = group.perm_fstats(Y, s0, W, s, scale)
    assert none is None and none2 is None and np.array_equal(kmax2, kmax)
    # f_first given without f_ref, f_ref given without f_first
    kmax3, none3, first3 = group.perm_fstats(Y, s0, W, s, scale, want_first=True)
    assert none3 is None and np.array_equal(first3, table[0]) and np.array_equal(kmax3, kmax)
    kmax4, count4, none4 = group.perm_fstats(Y, s0, W, s, scale, f_ref=f_ref)
    assert none4 is None and np.array_equal(count4, count) and np.array_equal(kmax4, kmax)
    # count accumulates: a second launch on top of the first doubles it
    _, twice, _ = group.perm_fstats(Y, s0, W, s, scale, f_ref=f_ref, count=count)
    assert np.array_equal(twice, 2 * count)


def test_count_is_left_alone_without_f_ref(group):
    cs = case(group, "n5_r2_s1_v63_k9")
    Yt, st, Wt = dev(cs["Y"]), dev(cs["s0"]), dev(cs["W"])
    cnt = torch.full((63,), 7, dtype=torch.int32, device="cuda")
    kmax = torch.empty(9, dtype=torch.float64, device="cuda")
    group._launch_f(torch.device("cuda", 0), Yt, st, Wt, cs["s"], cs["scale"], None, None, kmax, cnt)
    assert (cnt.cpu().numpy() == 7).all() and np.array_equal(kmax.cpu().numpy(), cs["table"].max(axis=1))


# ---------------------------------------------------------------- the bits depend on W[k], Y[:, v], s0[v], s and scale alone

@pytest.mark.parametrize("name", ["n12_r4_s2_v65_k32", "n12_r2_s2_v4096_kmax", "nmax_rmax_smax_tile_minus_1_kmax"])
def test_a_reordered_batch_and_reordered_voxels(group, name):
    cs = case(group, name)
    Y, s0, W, s, scale, table = cs["Y"], cs["s0"], cs["W"], cs["s"], cs["scale"], cs["table"]
    f_ref = table[0].copy()
    kmax, count, first = group.perm_fstats(Y, s0, W, s, scale, f_ref=f_ref, want_first=True)
    rng = np.random.default_rng(40)
    order = rng.permutation(W.shape[0])
    k2, c2, f2 = group.perm_fstats(Y, s0, W[order], s, scale, f_ref=f_ref, want_first=True)
    assert np.array_equal(k2, kmax[order]) and np.array_equal(c2, count) and np.array_equal(f2, table[order[0]])
    vox = rng.permutation(Y.shape[1])
    k3, c3, f3 = group.perm_fstats(Y[:, vox], s0[vox], W, s, scale, f_ref=f_ref[vox], want_first=True)
    assert np.array_equal(k3, kmax) and np.array_equal(c3, count[vox]) and np.array_equal(f3, first[vox])
    m = min(100, Y.shape[1])                                       # fewer voxels: the first 100 alone give their own bits
    _, c4, f4 = group.perm_fstats(Y[:, :m], s0[:m], W, s, scale, f_ref=f_ref[:m], want_first=True)
    assert np.array_equal(c4, count[:m]) and np.array_equal(f4, first[:m])


def test_k1_launches_against_one_launch_of_max_k(group):
    cs = case(group, "n12_r2_s2_v4096_kmax")
    Y, s0, W, s, scale, table = cs["Y"], cs["s0"], cs["W"], cs["s"], cs["scale"], cs["table"]
    f_ref = table[0].copy()
    kmax, count, _ = group.perm_fstats(Y, s0, W, s, scale, f_ref=f_ref)
    Yt, st, Wt, rt = dev(Y), dev(s0), dev(W), dev(f_ref)
    cnt = torch.zeros(4096, dtype=torch.int32, device="cuda")
    km = torch.empty(MAX_K, dtype=torch.float64, device="cuda")
    for k in range(MAX_K):
        group._launch_f(torch.device("cuda", 0), Yt, st, Wt[k:k + 1], s, scale, rt, None, km[k:k + 1], cnt)
    assert np.array_equal(km.cpu().numpy(), kmax) and np.array_equal(cnt.cpu().numpy().view(np.uint32), count)


SPLIT = (12, 3, 2, TILE + 1, 2 * MAX_K + 1, 1)                      # n, r, s, V, P, seed


def test_a_set_split_over_three_launches(group):
    n, r, s, V, P, seed = SPLIT
    Y, s0, W, scale = make_inputs(group, n, r, s, V, P, seed)
    preconditions(gf.perm_fstats(Y, s0, W, s, scale, None, LD))
    f_obs = group.perm_fstats(Y, s0, W[:1], s, scale, want_first=True)[2]
    want = gf.perm_fstats(Y, s0, W, s, scale, f_obs, np.float64)
    assert np.array_equal(f_obs, want["F"][0])
    count, kmax = None, []
    for k0 in range(0, P, MAX_K):                                  # 256 + 256 + 1
        km, count, _ = group.perm_fstats(Y, s0, W[k0:k0 + MAX_K], s, scale, f_ref=f_obs, count=count)
        kmax.append(km)
    assert len(kmax) == 3 and np.array_equal(np.concatenate(kmax), want["kmax"]) and np.array_equal(count, want["count"])


@pytest.mark.parametrize("name", ["n5_r1_s1_tile_plus_1_k8", "n12_r5_s2_v4096_k5", "n12_r2_s1_v65_k7"])
def test_negated_weights_give_the_same_bits(group, name):
    cs = case(group, name)
    assert np.array_equal(device_table(group, cs["Y"], cs["s0"], -cs["W"], cs["s"], cs["scale"]), cs["table"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_identity_fed_back_is_counted_in_every_voxel(group, name):
    cs = case(group, name)
    a = (cs["Y"], cs["s0"], cs["W"][:1], cs["s"], cs["scale"])
    first = group.perm_fstats(*a, want_first=True)[2]
    _, count, again = group.perm_fstats(*a, f_ref=first, want_first=True)
    assert np.array_equal(again, first) and (count == 1).all()


# ---------------------------------------------------------------- s = 1 against the t entry

@pytest.mark.parametrize("n,r,V,K,seed", [(12, 1, 65, 9, 1), (12, 3, TILE + 1, 32, 2), (MAX_N, MAX_R, 64, 5, 3)])
def test_one_column_f_is_the_t_entrys_t_squared(group, n, r, V, K, seed):
    rng = np.random.default_rng([seed, n, r, V, K])
    X = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, r - 1))], axis=1)
    c = np.zeros(r)
    c[0] = 1.0
    perms = group.permutation_set(X, c, K, seed, "flip")
    Wt, dof = group.weights(X, c, perms)
    Wf, s, dof_f = group.weights_f(X, c, perms)
    assert s == 1 and dof_f == dof and np.array_equal(Wf, Wt[:, 1:])
    Yr, s0 = group.residualise(rng.standard_normal((n, V)) + 0.3, X, c)
    assert gf.perm_fstats(Yr, s0, Wf, 1, float(dof), None, LD)["ratio"].min() >= 0.005
    F = np.stack([group.perm_fstats(Yr, s0, Wf[k:k + 1], 1, float(dof), want_first=True)[2] for k in range(K)])
    t = np.stack([group.perm_stats(Yr, s0, Wt[k:k + 1], want_first=True)[2] for k in range(K)])
    assert np.array_equal(F, gf.perm_f(Yr, s0, Wf, 1, float(dof))[0]) and np.array_equal(t, gn.perm_t(Yr, s0, Wt)[0])
    err = float(np.abs(F - t * t).max() / (t * t).max())
    print("|F - t^2| / max t^2: %.3g" % err)
    assert err <= bound() + bound("t", "group_parity.json")


# ---------------------------------------------------------------- edge values

def test_no_residual_gives_zero_and_a_nan_is_passed_over(group):
    cs = case(group, "n12_r4_s2_v65_k32")
    Y, s0, W, s, scale, table = cs["Y"].copy(), cs["s0"].copy(), cs["W"], cs["s"], cs["scale"], cs["table"]
    s0[3] = 0.0                                                    # rss = -q < 0
    s0[4] = -1.0
    Y[:, 5] = 0.0                                                  # q = 0, rss = s0 - 0 with s0 = 0: exactly 0
    s0[5] = 0.0
    Y[2, 7] = np.nan                                               # one NaN in a voxel's column: every F of that voxel is not a number
    f_ref = np.zeros(65)
    kmax, count, first = group.perm_fstats(Y, s0, W, s, scale, f_ref=f_ref, want_first=True)
    want = gf.perm_fstats(Y, s0, W, s, scale, f_ref, np.float64)
    assert (want["F"][:, [3, 4, 5]] == 0.0).all() and np.isnan(want["F"][:, 7]).all()
    assert (first[[3, 4, 5]] == 0.0).all() and not np.signbit(first[[3, 4, 5]]).any() and np.isnan(first[7])
    assert np.array_equal(first, want["F"][0], equal_nan=True) and np.array_equal(kmax, want["kmax"]) and np.array_equal(count, want["count"])
    assert count[7] == 0 and (count[[3, 4, 5]] == 32).all() and np.isfinite(kmax).all()
    others = np.delete(np.arange(65), [3, 4, 5, 7])
    assert np.array_equal(kmax, table[:, others].max(axis=1))      # the NaN voxel and the zeros change no maximum
    # every voxel NaN: -infinity
    kmax_nan, count_nan, first_nan = group.perm_fstats(np.full_like(Y, np.nan), s0, W, s, scale, f_ref=f_ref, want_first=True)
    assert (kmax_nan == -np.inf).all() and not count_nan.any() and np.isnan(first_nan).all()
    # a NaN in s0 alone
    s0n = cs["s0"].copy()
    s0n[0] = np.nan
    kmax_s, _, first_s = group.perm_fstats(cs["Y"], s0n, W, s, scale, want_first=True)
    assert np.isnan(first_s[0]) and np.array_equal(kmax_s, table[:, 1:].max(axis=1))


def raw(L, n, V, Y, s0, r, s, scale, K, W, f_ref, f_first, kmax, count):
    p = lambda t: None if t is None else t.data_ptr()
    return L.met2_group_perm_fstats(0, n, V, p(Y), p(s0), r, s, scale, K, p(W), p(f_ref), p(f_first), p(kmax), p(count), None)


def test_no_voxels_is_valid(group, L):
    Y, s0 = torch.empty((5, 0), dtype=torch.float64, device="cuda"), torch.empty(0, dtype=torch.float64, device="cuda")
    W, kmax = dev(np.ones((3, 2, 5))), torch.zeros(3, dtype=torch.float64, device="cuda")
    assert raw(L, 5, 0, Y, s0, 2, 1, 3.0, 3, W, None, None, kmax, None) == 0
    assert (kmax.cpu().numpy() == -np.inf).all()
    assert raw(L, 5, 0, None, None, 2, 2, 1.5, 3, W, None, None, kmax, None) == 0


# ---------------------------------------------------------------- limits and refusals

def test_refusals_come_before_any_device_work(group, L):
    Y, s0 = dev(np.ones((MAX_N, 8))), dev(np.ones(8))
    W = dev(np.ones((2, MAX_R, MAX_N)))
    kmax = torch.full((2,), 5.0, dtype=torch.float64, device="cuda")
    first = torch.full((8,), 5.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    names = ("n", "V", "Y", "s0", "r", "s", "scale", "K", "W", "f_ref", "f_first", "kmax", "count")
    ok = dict(zip(names, (MAX_N, 8, Y, s0, 2, 1, 3.0, 2, W, None, first, kmax, cnt)))

    def with_(**kw):
        a = dict(ok, **kw)
        return raw(L, *[a[k] for k in names])

    for kw in (dict(n=MAX_N + 1), dict(r=MAX_R + 1, s=1), dict(K=MAX_K + 1)):
        assert with_(**kw) == UNSUPPORTED and L.met2_last_error(), kw
    for kw in (dict(Y=None), dict(s0=None), dict(W=None), dict(kmax=None), dict(n=2, r=2), dict(n=1, r=1), dict(r=0), dict(K=0), dict(V=-1),
               dict(s=0), dict(s=-1), dict(s=3), dict(r=MAX_R, s=MAX_R + 1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")),
               dict(scale=float("inf")), dict(f_ref=s0, count=None)):
        assert with_(**kw) == INVALID and L.met2_last_error(), kw
    torch.cuda.synchronize()
    assert (kmax.cpu().numpy() == 5.0).all() and (first.cpu().numpy() == 5.0).all() and (cnt.cpu().numpy() == 7).all()
    assert with_() == 0 and not (kmax.cpu().numpy() == 5.0).any() and not (first.cpu().numpy() == 5.0).any()
    assert with_(r=2, s=2) == 0 and with_(f_ref=s0) == 0
    with pytest.raises(ValueError):
        group.perm_fstats(np.ones((4, 3)), np.ones(2), np.ones((1, 2, 4)), 1, 2.0)
    with pytest.raises(ValueError):
        group.perm_fstats(np.ones((4, 3)), np.ones(3), np.ones((1, 2, 4)), 3, 2.0)


def test_refused_spatial_calls_leave_the_outputs(group, L):
    p = lambda x: None if x is None else x.data_ptr()
    i3 = lambda d: (C.c_int32 * 3)(*d)
    n, V = 5, 10
    Y, s0, W = dev(np.ones((n, V))), dev(np.full(V, 9.0)), dev(np.ones((2, 2, n)) * 0.1)
    at, ref = dev(np.arange(V) * 2, torch.int32), dev(np.zeros(V))
    first, gmax, cnt = dev(np.full(V, 5.0)), dev(np.full(2, 5.0)), torch.full((V,), 7, dtype=torch.int32, device="cuda")
    gok = dict(n=n, V=V, Y=Y, s0=s0, r=2, s=1, scale=3.0, K=2, W=W, dims=(4, 3, 2), at=at, mode=0, dh=0.5, E=0.5, H=2.0, conn=6, ref=ref,
               first=first, kmax=gmax, count=cnt)

    def grp(**kw):
        a = dict(gok, **kw)
        return L.met2_group_perm_ftfce(0, a["n"], a["V"], p(a["Y"]), p(a["s0"]), a["r"], a["s"], a["scale"], a["K"], p(a["W"]), i3(a["dims"]),
                                       p(a["at"]), a["mode"], a["dh"], a["E"], a["H"], a["conn"], p(a["ref"]), p(a["first"]), p(a["kmax"]),
                                       p(a["count"]), None, 0, None)

    descending = dev(np.arange(V)[::-1] * 2, torch.int32)
    beyond = dev(np.arange(V) + 20, torch.int32)
    for kw in (dict(s=0), dict(s=3), dict(scale=0.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(dh=0.0), dict(dh=float("nan")),
               dict(E=0.0), dict(H=-1.0), dict(conn=8), dict(mode=2), dict(K=0), dict(dims=(0, 3, 2)), dict(Y=None), dict(s0=None), dict(W=None),
               dict(at=None), dict(kmax=None), dict(count=None), dict(r=0), dict(n=2), dict(V=0), dict(V=25), dict(at=descending),
               dict(at=beyond)):
        assert grp(**kw) == INVALID and L.met2_last_error(), kw
    for kw in (dict(K=TFCE_MAX_K + 1), dict(n=MAX_N + 1), dict(r=MAX_R + 1, n=20)):
        assert grp(**kw) == UNSUPPORTED and L.met2_last_error(), kw
    torch.cuda.synchronize()
    assert (first.cpu().numpy() == 5.0).all() and (gmax.cpu().numpy() == 5.0).all() and (cnt.cpu().numpy() == 7).all()
    assert grp() == 0 and (cnt.cpu().numpy() > 7).all() and not (gmax.cpu().numpy() == 5.0).any()
    with pytest.raises(ValueError):
        group.perm_ftfce(np.ones((4, 3)), np.ones(3), np.ones((1, 2, 4)), 1, 2.0, (2, 2, 2), np.arange(2), dh=0.5)


# ---------------------------------------------------------------- the spatial entry

GRID, N_MASK, SPATIAL = (12, 10, 8), 700, (12, 3, 2, 11)            # the grid, its tested voxels; n, r, s, seed


def spatial_inputs(group):
    """32 candidates on 700 voxels of the 12 x 10 x 8 grid, with a smooth mean so that supports have some extent"""
    if "spatial" not in _CACHE:
        n, r, s, seed = SPATIAL
        rng = np.random.default_rng([seed, n, r, s])
        X = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, r - 1))], axis=1)
        Cm = np.eye(r)[:, :s]
        perms = group.permutation_set(X, Cm, TFCE_MAX_K, seed, "flip")
        W, _, dof = group.weights_f(X, Cm, perms)
        at = np.sort(rng.choice(int(np.prod(GRID)), N_MASK, replace=False)).astype(np.int32)
        mean = ndimage.uniform_filter(rng.standard_normal(GRID), 3).reshape(-1)[at] * 2.0 + 0.3
        Yr, s0 = group.residualise(rng.standard_normal((n, N_MASK)) + mean[None, :], X, Cm)
        scale = float(dof) / s
        preconditions(gf.perm_fstats(Yr, s0, W, s, scale, None, LD))
        f_dev = np.stack([group.perm_fstats(Yr, s0, W[k:k + 1], s, scale, want_first=True)[2] for k in range(TFCE_MAX_K)])
        assert np.array_equal(f_dev, gf.perm_f(Yr, s0, W, s, scale)[0])
        _CACHE["spatial"] = (Yr, s0, W, s, scale, at, f_dev)
    return _CACHE["spatial"]


@pytest.mark.parametrize("mode,conn", [("tfce", 6), ("tfce", 26), ("extent", 6), ("extent", 26)])
def test_spatial_entry_equals_tfce_of_the_f_maps_and_the_restatement(group, mode, conn):
    Y, s0, W, s, scale, at, f_dev = spatial_inputs(group)
    step = float(f_dev[0].max()) / 100.0 if mode == "tfce" else 2.0
    assert step > 0
    maps, mask = tn.dense(f_dev, GRID, at)
    s_dev = group.spatial(maps, mask, mode, step, connectivity=conn)[0].reshape(TFCE_MAX_K, -1)[:, at]      # met2_tfce on the device's F maps
    ref = s_dev[0].copy()
    full = gf.perm_fspatial(Y, s0, W, s, scale, GRID, at, mode, step, 0.5, 2.0, conn, ref)
    assert np.array_equal(s_dev, full["s"])
    for K in (1, 5, TFCE_MAX_K):
        kmax, count, first = group.perm_ftfce(Y, s0, W[:K], s, scale, GRID, at, mode, step, connectivity=conn, ref=ref, want_first=True)
        assert np.array_equal(first, ref) and np.array_equal(kmax, s_dev[:K].max(axis=1)) and np.array_equal(kmax, full["kmax"][:K])
        assert count.dtype == np.uint32 and np.array_equal(count, (s_dev[:K] >= ref[None, :]).sum(axis=0))
        # ref NULL: no count; first NULL: the same kmax; count accumulates
        kmax2, none, none2 = group.perm_ftfce(Y, s0, W[:K], s, scale, GRID, at, mode, step, connectivity=conn)
        assert none is None and none2 is None and np.array_equal(kmax2, kmax)
        _, twice, _ = group.perm_ftfce(Y, s0, W[:K], s, scale, GRID, at, mode, step, connectivity=conn, ref=ref, count=count)
        assert np.array_equal(twice, 2 * count)
    assert np.array_equal(count, full["count"])
    # a row does not depend on its place or its mates: the batch reversed, and five rows from its middle
    k_rev, c_rev, f_rev = group.perm_ftfce(Y, s0, W[::-1], s, scale, GRID, at, mode, step, connectivity=conn, ref=ref, want_first=True)
    assert np.array_equal(k_rev, kmax[::-1]) and np.array_equal(c_rev, count) and np.array_equal(f_rev, s_dev[-1])
    k_mid, _, f_mid = group.perm_ftfce(Y, s0, W[13:18], s, scale, GRID, at, mode, step, connectivity=conn, want_first=True)
    assert np.array_equal(k_mid, kmax[13:18]) and np.array_equal(f_mid, s_dev[13])


# ---------------------------------------------------------------- end to end

def test_group_stats_filter_gives_the_host_run(group):
    motor = importlib.import_module(PKG + ".motor")
    Y, X, fc, grid, at, block, near, host = gf.planted_host(group)
    out = motor.group_stats_filter(Y.reshape((Y.shape[0],) + grid), X, f_contrast=fc, n_perm=400, seed=0, tfce=True)
    assert "tstat" not in out and "cope" not in out
    for key in ("fstat", "p_uncorrected", "p_fwe", "count", "tfce", "p_tfce_uncorrected", "p_tfce_fwe", "tfce_count"):
        assert out[key].shape == grid and np.array_equal(out[key].reshape(-1), host[key]), key
    for key in ("max_dist", "tfce_max_dist"):
        assert np.array_equal(out[key], host[key]), key
    for key in ("dh", "tfce_crit", "f_crit", "dof", "n_perm", "exhaustive", "tfce_options"):
        assert out[key] == host[key], key
    assert sorted(set(out) - {"mask"}) == sorted(host)
    found = out["p_tfce_fwe"].reshape(-1) <= 0.05
    assert found[block].sum() >= 108 and not found[~near].any()
    # the cluster extent on F, in small batches
    ext = motor.group_stats_filter(Y.reshape((Y.shape[0],) + grid), X, f_contrast=fc, n_perm=64, seed=0, cluster_threshold=8.0,
                                   work_bytes=group.tfce_work_bytes(3, grid, Y.shape[1]))
    want = group.randomise(Y, X, f_contrast=fc, n_perm=64, seed=0, batch_stat=gf.batch_stat, batch_spatial=gf.batch_spatial,
                           cluster_threshold=8.0, grid=grid, at=at)
    for key in ("fstat", "cluster_extent", "p_cluster_fwe", "cluster_count"):
        assert np.array_equal(ext[key].reshape(-1), want[key]), key
    assert np.array_equal(ext["cluster_max_dist"], want["cluster_max_dist"])


# ---------------------------------------------------------------- the t entry, which shares the header of the kernels, keeps its bits

def test_the_t_entry_keeps_its_bits_beside_the_f_entry(group):
    n, r, V, K, two_sided, seed = 12, 2, 65, 2, True, 10          # tests/test_gpu_group.py's case n12_r2_v65_k2_abs, restated
    rng = np.random.default_rng([seed, n, r, V, K])
    X = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, r - 1))], axis=1)
    c = np.zeros(r)
    c[0] = 1.0
    perms = group.permutation_set(X, c, K, seed, "flip")
    W, dof = group.weights(X, c, perms)
    Yr, s0 = group.residualise(rng.standard_normal((n, V)) + 0.3, X, c)
    Wf = np.ascontiguousarray(W[:, 1:])
    f_first = group.perm_fstats(Yr, s0, Wf, 1, float(dof), want_first=True)[2]           # the F launch first, then the t launch
    assert np.array_equal(f_first, gf.perm_f(Yr, s0, Wf, 1, float(dof))[0][0])
    want = gn.perm_stats(Yr, s0, W, two_sided, None, np.float64)
    t_ref = want["t"][0].copy()
    kmax, count, first = group.perm_stats(Yr, s0, W, two_sided, t_ref=t_ref, want_first=True)
    assert np.array_equal(first, want["t"][0]) and np.array_equal(kmax, want["kmax"])
    assert np.array_equal(count, gn.perm_stats(Yr, s0, W, two_sided, t_ref, np.float64)["count"])
