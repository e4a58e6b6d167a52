"""GPU tests of met2_tissue_segment and its stage entries (csrc/met2_seg.hip), motor.tissue_segment_filter and segment='yes' in the drivers,
against the numpy restatement of the algorithm (tests/tools/seg_numpy.py, which follows include/met2_hip.h step by step).

Stages.  The labelling is discrete, so the stage tests ask for EQUAL labels in every voxel.  What allows it: the restatement is handed the
device's own constants (mu_k, a_k, h_k), and every operation of an energy rounds once on the device as in numpy, so both compare the same
bits.  The constants themselves: a_k = 1 / (2 var_k) is one division (exact against numpy), h_k = log(var_k) / 2 within 2 ulp (the device's log
is not numpy's).  Posteriors within 1e-12 of the restatement (the device's exp against numpy's, on arguments that are the same bits), rows
summing to 1 within 4 ulp (K <= 8 quotients of one sum), and the partial sums equal to the bit to the same terms added on the host in the
kernels' order.
Shapes: the tile of seg_icm_kernel is TILE = 4 x 8 x 16 voxels; the shapes put its seams strictly inside the volume on every axis, are odd
on every axis, or have one or two axes of length 1.

Whole filter.  Labels equal in every voxel, posteriors within 1e-9 absolute, classes within 1e-9 relative (the bar the bias filter's classes
are pinned at, for the same sums).  tests/test_seg_host.py is what allows equal labels: on these volumes and seeds the fp64 and the
long-double restatement agree in every voxel, so no label hangs on a rounding.  Measured figures: profiles/seg_parity.json."""
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
import bias_numpy as bn                                            # noqa: E402
import seg_numpy as sn                                             # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
TILE = (4, 8, 16)                                                  # seg_icm_kernel's tile (x, y, z)
EPS = np.finfo(np.float64).eps


def record(name, figures):
    """with MET2_SEG_PARITY_JSON set, the measured deviations are kept in that file (profiles/seg_parity.json was written this way)"""
    path = os.environ.get("MET2_SEG_PARITY_JSON")
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
def seg(motor):
    return importlib.import_module(PKG + ".seg")


# ---- the stages ----

def levels_for(K):
    return sn.LEVELS if K <= 3 else tuple(np.geomspace(400.0, 1600.0, K))


# name: shape, voxel size, K, mask kind, beta, index of a dead class or None, start from random labels
T = TILE
STAGE_CASES = {
    "block": ((24, 20, 18), (1.0, 1.0, 1.0), 3, "all", 0.1, None, False),      # the issue's five shapes
    "odd": ((17, 9, 5), (1.0, 1.0, 1.0), 3, "all", 0.1, None, False),
    "slab": ((33, 1, 7), (1.0, 1.0, 1.0), 3, "all", 0.1, None, False),
    "line": ((1, 1, 64), (1.0, 1.0, 1.0), 2, "all", 0.3, None, False),
    "flat": ((16, 16, 1), (1.0, 1.0, 1.0), 3, "all", 0.1, None, False),
    "tile+1": ((T[0] + 1, T[1] + 1, T[2] + 1), (1.0, 1.0, 1.0), 3, "all", 0.1, None, True),      # one voxel past a seam on every axis
    "2tile+1": ((2 * T[0] + 1, 2 * T[1] + 1, 2 * T[2] + 1), (1.0, 1.0, 1.0), 3, "holes", 0.1, None, True),
    "holes": ((24, 20, 18), (1.0, 1.0, 1.0), 3, "holes", 0.1, None, False),
    "aniso": ((17, 9, 5), (1.0, 1.0, 3.0), 3, "all", 0.2, None, True),
    "k1": ((17, 9, 5), (1.0, 1.0, 1.0), 1, "all", 0.1, None, False),
    "k2": ((17, 9, 5), (1.0, 1.0, 1.0), 2, "holes", 0.1, None, True),
    "k4": ((24, 20, 18), (1.0, 1.0, 1.0), 4, "all", 0.1, None, True),
    "k8": ((24, 20, 18), (1.0, 1.0, 1.0), 8, "disc", 0.1, None, True),
    "dead": ((24, 20, 18), (2.0, 1.0, 1.0), 3, "holes", 0.1, 1, True),
    "beta0": ((17, 9, 5), (1.0, 1.0, 1.0), 3, "all", 0.0, None, True),
    "bigbeta": ((24, 20, 18), (1.0, 1.0, 1.0), 3, "all", 5.0, None, True),
}


def test_the_shapes_cross_the_tile_seams(seg):
    assert seg.TILE == TILE
    shapes = [c[0] for c in STAGE_CASES.values()]
    for want in ((24, 20, 18), (17, 9, 5), (33, 1, 7), (1, 1, 64), (16, 16, 1)):
        assert want in shapes
    for ax in range(3):                                                  # a seam strictly inside, two seams, and a last tile of one voxel
        assert any(s[ax] > TILE[ax] for s in shapes) and any(s[ax] > 2 * TILE[ax] for s in shapes)
        assert any(s[ax] % TILE[ax] == 1 and s[ax] > TILE[ax] for s in shapes)
    assert all(n > t for n, t in zip((24, 20, 18), TILE))                # 24 x 20 x 18 has seams inside on all three axes at once


@functools.lru_cache(maxsize=None)
def stage_case(name):
    """-> dict(y, om, idx, classes [3 K], mu, w, beta, K, start: random labels on the domain or None): computed once, never written to"""
    shape, vox, K, kind, beta, dead, random_start = STAGE_CASES[name]
    seed = 100 + sorted(STAGE_CASES).index(name)
    v, mask, _ = sn.phantom(shape, seed, levels=levels_for(K), mask_kind=kind)
    y, om = bn.log_domain(v, mask)
    ini = bn.init_classes(y[om], K)
    mu, var, pi = ini["mu"], ini["var"], ini["pi"]
    for _ in range(3):
        bn.m_step(bn.e_step(y[om], mu, var, pi), y[om], mu, var, pi)
    if dead is not None:
        pi[dead] = 0.0
    rng = np.random.default_rng(seed)
    start = None
    if random_start:
        alive = np.flatnonzero(pi != 0)
        start = np.where(om, alive[rng.integers(0, len(alive), size=shape)], sn.OFF).astype(np.uint8)
    out = {"y": y, "om": om, "idx": np.flatnonzero(om.reshape(-1)).astype(np.int32), "classes": np.concatenate([mu, var, pi]), "mu": mu,
           "w": sn.axis_weights(vox), "beta": beta, "K": K, "start": start, "dead": dead}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def test_seg_consts(seg):
    var = np.array([1e-6, 3.7e-3, 0.25, 1.0, 7.5, 1e-6 * (1 + 2 ** -50), 0.0123456789, 2.0 ** -20])
    pi = np.array([0.2, 0.0, 0.1, 0.1, 0.0, 0.2, 0.2, 0.2])
    a, h, live = seg.seg_consts(np.concatenate([np.linspace(5.0, 7.0, 8), var, pi]))
    assert np.array_equal(a, 1.0 / (2.0 * var))
    ref = 0.5 * np.log(var)
    ulps = np.abs(h - ref) / np.spacing(np.abs(ref))
    print("h_k: %.2f ulp" % ulps.max())
    record("consts", {"h_ulp": float(ulps.max())})
    assert ulps.max() <= 2.0
    assert np.array_equal(live, pi != 0) and live.dtype == bool
    a1, h1, l1 = seg.seg_consts([6.0, 0.5, 1.0])
    assert a1.tolist() == [1.0] and l1.tolist() == [True] and abs(h1[0] - 0.5 * np.log(0.5)) <= 2 * np.spacing(0.35)


def where_differs(got, ref, c, a, h, live):
    """the assertion message when labels differ: where, and the restatement's energy gap there"""
    bad = np.argwhere(got != ref)
    if len(bad) == 0:
        return ""
    gap = sn.energy_gap(ref, c["y"], c["mu"], a, h, live, c["w"], c["beta"])
    i = tuple(bad[0])
    return "%d labels differ, the first at %s: device %d, restatement %d, the restatement's energy gap there %.3e (smallest over those %.3e)" % (
        len(bad), i, got[i], ref[i], gap[i], min(gap[tuple(b)] for b in bad))


@pytest.mark.parametrize("name", STAGE_CASES)
def test_init_and_icm_give_the_restatements_labels(seg, name):
    c = stage_case(name)
    a, h, live = seg.seg_consts(c["classes"])                           # the device's constants go to the restatement
    args = (c["y"], c["mu"], a, h, live, c["w"], c["beta"])
    lab0 = seg.seg_init(c["y"], c["idx"], c["classes"])
    ref0 = sn.init_labels(c["y"], c["om"], c["mu"], a, h, live)
    assert lab0.dtype == np.uint8 and np.array_equal(lab0, ref0), where_differs(lab0, ref0, dict(c, beta=0.0), a, h, live)
    assert np.all(lab0[~c["om"]] == sn.OFF) and lab0[c["om"]].max() < c["K"]
    start = lab0 if c["start"] is None else c["start"]
    # one colour pass, the other colour after it, one sweep, eight sweeps
    p0 = seg.seg_icm(start, c["y"], c["classes"], c["w"], c["beta"], 1, colour=0)
    r0 = sn.icm_pass(start, *args, 0)
    assert np.array_equal(p0, r0), where_differs(p0, r0, c, a, h, live)
    colour = sn.colour_of(start.shape)
    assert np.array_equal(p0[colour == 1], start[colour == 1])           # the other colour is not touched
    p1 = seg.seg_icm(p0, c["y"], c["classes"], c["w"], c["beta"], 1, colour=1)
    r1 = sn.icm_pass(r0, *args, 1)
    assert np.array_equal(p1, r1), where_differs(p1, r1, c, a, h, live)
    s1 = seg.seg_icm(start, c["y"], c["classes"], c["w"], c["beta"], 1)
    assert np.array_equal(s1, r1), where_differs(s1, r1, c, a, h, live)
    s8 = seg.seg_icm(start, c["y"], c["classes"], c["w"], c["beta"], 8)
    r8 = sn.icm(start, *args, 8)
    assert np.array_equal(s8, r8), where_differs(s8, r8, c, a, h, live)
    assert np.array_equal(seg.seg_icm(start, c["y"], c["classes"], c["w"], c["beta"], 0), start)
    changed = float((s1 != start)[c["om"]].mean())
    print("%s: one sweep changes %.1f %% of the labels, eight %.1f %%" % (name, 100 * changed, 100 * float((s8 != start)[c["om"]].mean())))
    assert np.all(s8[~c["om"]] == sn.OFF)
    if c["dead"] is not None:
        assert not (s8 == c["dead"]).any() and not (lab0 == c["dead"]).any()
    if name == "beta0":
        assert np.array_equal(s1, lab0) and np.array_equal(s8, lab0)     # without a prior every visit is the plain argmin
    if name == "bigbeta":
        assert changed > 0.3 and sn.isolated(s1) < sn.isolated(start)    # one sweep recolours the block: the start is random labels
    if name == "k1":
        assert np.all(s8[c["om"]] == 0)


def test_icm_takes_tensors_and_leaves_its_input(seg):
    c = stage_case("odd")
    lab0 = seg.seg_init(c["y"], c["idx"], c["classes"])
    yt = torch.as_tensor(c["y"], device="cuda")
    lt = torch.as_tensor(lab0, device="cuda")
    out = seg.seg_icm(lt, yt, c["classes"], c["w"], c["beta"], 2)
    assert torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8
    assert np.array_equal(lt.cpu().numpy(), lab0)
    assert np.array_equal(out.cpu().numpy(), seg.seg_icm(lab0, c["y"], c["classes"], c["w"], c["beta"], 2))
    t0 = seg.seg_init(yt, c["idx"], c["classes"])
    assert torch.is_tensor(t0) and np.array_equal(t0.cpu().numpy(), lab0)
    with pytest.raises(ValueError):
        seg.seg_icm(np.full(lab0.shape, 3, dtype=np.uint8), c["y"], c["classes"])      # a label that is no class
    with pytest.raises(ValueError):
        seg.seg_icm(lab0, c["y"], c["classes"], colour=2)


@pytest.mark.parametrize("name", ["block", "holes", "aniso", "dead", "k8", "k1", "line"])
def test_posterior(seg, name):
    c = stage_case(name)
    K = c["K"]
    a, h, live = seg.seg_consts(c["classes"])
    args = (c["y"], c["mu"], a, h, live, c["w"], c["beta"])
    lab = sn.icm(sn.init_labels(c["y"], c["om"], c["mu"], a, h, live) if c["start"] is None else c["start"], *args, 2)
    got = seg.seg_posterior(lab, c["y"], c["idx"], c["classes"], c["w"], c["beta"])
    p = got["prob"]
    ref = sn.posterior(lab, *args)
    e = float(np.abs(p - ref).max())
    rows = float(np.abs(p.sum(axis=0)[c["om"]] - 1.0).max())
    print("%s: max |p - ref| = %.3e, rows sum to 1 within %.2f ulp" % (name, e, rows / EPS))
    record("posterior_" + name, {"shape": list(lab.shape), "prob_abs": e, "row_sum_ulp": rows / EPS})
    assert p.shape == (K,) + lab.shape and p.dtype == np.float64
    assert e <= 1e-12
    assert rows <= 4 * EPS
    assert np.all(p[:, ~c["om"]] == 0.0) and np.all(p >= 0.0)
    if c["dead"] is not None:
        assert np.all(p[c["dead"]] == 0.0)
    # the partial sums: the same terms, from the device's own posteriors, added on the host in the kernels' order
    u = c["y"].reshape(-1)[c["idx"]]
    pl = p.reshape(K, -1)[:, c["idx"]]
    d = u[None, :] - c["mu"][:, None]
    terms = np.stack([pl, pl * u[None, :], (pl * d) * d])
    part = seg.chunk_sums(terms)
    assert got["part"].shape == part.shape == (3, K, -(-len(u) // 1024))
    assert np.array_equal(got["part"], part)
    assert np.array_equal(got["sums"], seg.partial_sum(part))
    assert np.abs(got["sums"][0].sum() - len(u)) <= 1e-12 * len(u)


def test_finish_ranks_by_mean(seg):
    rng = np.random.default_rng(5)
    K, shape = 5, (7, 6, 5)
    mu = np.array([6.5, 6.1, 6.5, 5.9, 7.0])                            # a tie: the lower index ranks first
    classes = np.concatenate([mu, np.linspace(0.01, 0.05, K), [0.3, 0.0, 0.2, 0.3, 0.2]])
    lab = rng.integers(0, K, size=shape).astype(np.uint8)
    lab[rng.random(shape) < 0.2] = sn.OFF
    praw = rng.random((K,) + shape)
    s, p, cl = seg.seg_finish(lab, praw, classes)
    rs, rp, rc = sn.finish(lab, praw, mu, classes[K:2 * K], classes[2 * K:])
    assert s.dtype == np.uint8 and np.array_equal(s, rs) and np.array_equal(p, rp) and np.array_equal(cl, rc)
    assert sn.ranks(mu).tolist() == [2, 1, 3, 0, 4]
    s2, p2, _ = seg.seg_finish(lab, None, classes)
    assert p2 is None and np.array_equal(s2, rs)


# ---- the whole filter ----

@functools.lru_cache(maxsize=None)
def reference(name):
    """(v, mask, voxel size, kwargs, restatement's result) of a committed case: computed once, shared, never written to"""
    v, mask, vox, kw = sn.case(name)
    res = sn.tissue_segment(v, mask, vox, **kw)
    for a in (v, mask) + tuple(res.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v, mask, vox, kw, res


@pytest.mark.parametrize("name", sn.CASES)
def test_parity_with_the_restatement(motor, name):
    v, mask, vox, kw, ref = reference(name)
    K = kw.get("n_class", 3)
    s, p, classes = motor.tissue_segment_filter(v, mask, vox, **kw)
    assert s.dtype == np.uint8 and s.shape == v.shape and p.shape == (K,) + v.shape and p.dtype == np.float64 and classes.shape == (3 * K,)
    msg = ""
    if not np.array_equal(s, ref["seg"]):
        bad = np.argwhere(s != ref["seg"])
        gap = sn.energy_gap(ref["labels"], ref["y"], ref["mu"], ref["a"], ref["h"], ref["live"], ref["w"], kw.get("beta", 0.1))
        i = tuple(bad[0])
        msg = "%d labels differ, the first at %s: device %d, restatement %d; the restatement's energy gap there %.3e, the smallest over those %.3e" % (
            len(bad), i, s[i], ref["seg"][i], gap[i], min(gap[tuple(b)] for b in bad))
    e_prob = float(np.abs(p - ref["prob"]).max())
    live = ref["classes"] != 0
    e_cls = float(np.abs(classes[live] / ref["classes"][live] - 1.0).max())
    print("%s %s: %d labels differ, max |prob - ref| = %.3e, classes %.3e" % (name, v.shape, int((s != ref["seg"]).sum()), e_prob, e_cls))
    record(name, {"shape": list(v.shape), "labels_differ": int((s != ref["seg"]).sum()), "prob_abs": e_prob, "classes_rel": e_cls})
    assert np.array_equal(s, ref["seg"]), msg
    assert e_prob <= 1e-9
    assert e_cls <= 1e-9 and np.array_equal(classes[~live], ref["classes"][~live])
    on = s > 0
    assert np.array_equal(on, bn.domain(v, mask)) and np.all(p[:, ~on] == 0.0)
    assert np.abs(p.sum(axis=0)[on] - 1.0).max() <= 4 * EPS
    assert np.all(np.diff(classes[:K]) >= 0)


def test_deterministic_and_independent_of_the_embedding(motor):
    v, mask, vox, kw, ref = reference("holes")
    a = motor.tissue_segment_filter(v, mask, vox)
    b = motor.tissue_segment_filter(v, mask, vox)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    big_v = np.pad(v, 1, constant_values=123.0)
    big_m = np.pad(mask, 1, constant_values=0)
    s, p, classes = motor.tissue_segment_filter(big_v, big_m, vox)
    inner = (slice(1, -1),) * 3
    assert np.array_equal(s[inner], a[0]) and np.array_equal(p[(slice(None),) + inner], a[1]) and np.array_equal(classes, a[2])
    assert s.sum() == a[0].sum() and p.sum() == a[1].sum()               # nothing in the margin


def test_inverting_the_contrast_turns_the_labels_round(motor):
    """classes are numbered by ascending mean.  Both runs equal the restatement (test_parity_with_the_restatement), which puts more than 97 %
    of the voxels in their true tissue either way (tests/test_seg_host.py), so the two agree on at least 94 %."""
    v, mask, vox, _, _ = reference("block")
    vi = reference("inverted")[0]
    _, _, truth = sn.phantom(sn.CASES["block"][0], sn.CASES["block"][2])
    s, _, c = motor.tissue_segment_filter(v, mask, vox)
    si, _, ci = motor.tissue_segment_filter(vi, mask, vox)
    assert (s == truth + 1).mean() > 0.97 and (si == 3 - truth).mean() > 0.97
    assert (si == 4 - s).mean() >= 0.94
    assert np.all(np.diff(c[:3]) > 0) and np.all(np.diff(ci[:3]) > 0)
    for seg_, vol in ((s, v), (si, vi)):                                 # label 1 is the driest, 3 the wettest
        m = [np.log(vol[seg_ == l]).mean() for l in (1, 2, 3)]
        assert m[0] < m[1] < m[2]


def test_faces_null_outputs_and_degenerate_volumes(motor):
    v, mask, vox, kw, ref = reference("odd")
    s, p, classes = motor.tissue_segment_filter(v, mask, vox)
    plain = motor.tissue_segment_filter(v, mask, vox, return_prob=False)    # prob = classes = NULL
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, s)
    t = motor.tissue_segment_filter(torch.as_tensor(v, device="cuda"), None, vox)
    assert all(torch.is_tensor(x) and x.is_cuda for x in t)
    for x, y in zip(t, (s, p, classes)):
        assert np.array_equal(x.cpu().numpy(), y)
    pkg = importlib.import_module(PKG)
    assert pkg.tissue_segment_filter is motor.tissue_segment_filter
    L = importlib.import_module(PKG + "._lib").lib()
    dd = torch.as_tensor(v, device="cuda").contiguous()
    vx = (ctypes.c_double * 3)(*vox)
    nx, ny, nz = dd.shape
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
        so = torch.full(dd.shape, 99, dtype=torch.uint8, device="cuda")
        po = torch.full((3,) + tuple(dd.shape), 99.0, dtype=torch.float64, device="cuda")
        co = torch.full((9,), 99.0, dtype=torch.float64, device="cuda")
        assert L.met2_tissue_segment(0, nx, ny, nz, dd.data_ptr(), None, vx, 3, 0.1, 4, 10, 8, so.data_ptr() if want[0] else None,
                                     po.data_ptr() if want[1] else None, co.data_ptr() if want[2] else None, None) == 0
        assert np.array_equal(so.cpu().numpy(), s) if want[0] else bool((so == 99).all())
        assert np.array_equal(po.cpu().numpy(), p) if want[1] else bool((po == 99.0).all())
        assert np.array_equal(co.cpu().numpy(), classes) if want[2] else bool((co == 99.0).all())
    # the degenerate volumes: an empty mask, a constant volume
    some = np.zeros(v.shape, dtype=np.uint8)
    some[2:9, 1:5] = 1
    for vol, m, mu in ((v, np.zeros(v.shape, dtype=np.uint8), 0.0), (np.full(v.shape, 750.0), some, np.log(750.0))):
        so, po, co = motor.tissue_segment_filter(vol, m, vox)
        assert np.array_equal(so, m) and np.array_equal(po[0], m.astype(np.float64)) and np.all(po[1:] == 0.0)
        assert np.allclose(co[:3], mu, rtol=1e-15, atol=0.0) and np.all(co[3:6] == 0.0) and np.all(co[6:] == 1.0 / 3.0)
    # non-finite and non-positive voxels are left out
    vb = v.copy()
    vb[3, 3, 2], vb[4, 4, 1], vb[5, 5, 3], vb[6, 6, 0] = np.nan, np.inf, 0.0, -5.0
    sb = motor.tissue_segment_filter(vb, None, vox, return_prob=False)
    assert sb[3, 3, 2] == sb[4, 4, 1] == sb[5, 5, 3] == sb[6, 6, 0] == 0 and (sb == 0).sum() == 4


def test_return_codes(motor):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    dd = torch.full((8, 8, 8), 5.0, dtype=torch.float64, device="cuda")
    so = torch.full((8, 8, 8), 77, dtype=torch.uint8, device="cuda")
    po = torch.full((8, 8, 8, 8), 7.0, dtype=torch.float64, device="cuda")      # room for K = 8
    co = torch.full((24,), 7.0, dtype=torch.float64, device="cuda")

    def call(nx=8, ny=8, nz=8, v=dd, vox=(2.0, 2.0, 2.0), K=3, beta=0.1, n_outer=4, n_em=10, n_icm=8):
        return L.met2_tissue_segment(0, nx, ny, nz, None if v is None else v.data_ptr(), None, None if vox is None else (ctypes.c_double * 3)(*vox),
                                     K, beta, n_outer, n_em, n_icm, so.data_ptr(), po.data_ptr(), co.data_ptr(), None)

    assert call(v=None) == E_INVALID
    assert call(nx=-1) == E_INVALID and call(ny=-1) == E_INVALID and call(nz=-1) == E_INVALID
    assert call(K=0) == E_INVALID and call(n_outer=-1) == E_INVALID and call(n_em=0) == E_INVALID and call(n_icm=-1) == E_INVALID
    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        assert call(beta=bad) == E_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(vox=(bad, 2.0, 2.0)) == E_INVALID and call(vox=(2.0, 2.0, bad)) == E_INVALID
    assert call(vox=None) == E_INVALID
    assert call(K=9) == E_UNSUPPORTED
    assert call(nx=2048, ny=1024, nz=1024) == E_UNSUPPORTED            # 2^31 voxels; nothing is read
    for shape in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert call(*shape) == 0
    assert call(0, 8, 8, v=None) == 0
    assert call(0, 8, 8, K=0) == E_INVALID and call(0, 8, 8, beta=-1.0) == E_INVALID
    torch.cuda.synchronize()
    assert bool((so == 77).all()) and bool((po == 7.0).all()) and bool((co == 7.0).all())      # nothing was launched
    assert call(K=8) == 0 and call(n_outer=0) == 0 and call(n_icm=0) == 0 and call(beta=0.0) == 0
    assert bool((so == 1).all())                                       # a constant volume: degenerate
    # the stage entries
    y = torch.zeros(8, dtype=torch.float64, device="cuda")
    idx = torch.arange(8, dtype=torch.int32, device="cuda")
    lab = torch.full((8,), 77, dtype=torch.uint8, device="cuda")
    cl = (ctypes.c_double * 6)(6.0, 7.0, 0.1, 0.1, 0.5, 0.5)
    w = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    bad_var = (ctypes.c_double * 6)(6.0, 7.0, 0.0, 0.1, 0.5, 0.5)
    assert L.met2_seg_consts(0, 0, cl, None, None, None, None) == E_INVALID and L.met2_seg_consts(0, 9, cl, None, None, None, None) == E_UNSUPPORTED
    assert L.met2_seg_consts(0, 2, bad_var, None, None, None, None) == E_INVALID and L.met2_seg_consts(0, 2, None, None, None, None, None) == E_INVALID
    assert L.met2_seg_init(0, 0, y.data_ptr(), idx.data_ptr(), 0, 2, cl, lab.data_ptr(), None) == E_INVALID
    assert L.met2_seg_init(0, 8, y.data_ptr(), idx.data_ptr(), 9, 2, cl, lab.data_ptr(), None) == E_INVALID
    assert L.met2_seg_init(0, 8, None, idx.data_ptr(), 8, 2, cl, lab.data_ptr(), None) == E_INVALID
    assert L.met2_seg_icm(0, 2, 2, 0, lab.data_ptr(), y.data_ptr(), 2, cl, w, 0.1, 1, -1, None) == E_INVALID
    assert L.met2_seg_icm(0, 2, 2, 2, lab.data_ptr(), y.data_ptr(), 2, cl, w, -0.1, 1, -1, None) == E_INVALID
    assert L.met2_seg_icm(0, 2, 2, 2, lab.data_ptr(), y.data_ptr(), 2, cl, w, 0.1, -1, -1, None) == E_INVALID
    assert L.met2_seg_icm(0, 2, 2, 2, lab.data_ptr(), y.data_ptr(), 2, cl, w, 0.1, 1, 2, None) == E_INVALID
    assert L.met2_seg_icm(0, 2, 2, 2, lab.data_ptr(), y.data_ptr(), 2, cl, None, 0.1, 1, -1, None) == E_INVALID
    assert L.met2_seg_posterior(0, 2, 2, 2, lab.data_ptr(), y.data_ptr(), idx.data_ptr(), 0, 2, cl, w, 0.1, None, None, None) == E_INVALID
    assert L.met2_seg_finish(0, 8, None, None, 2, cl, lab.data_ptr(), None, None, None) == E_INVALID
    assert L.met2_seg_finish(0, 8, lab.data_ptr(), None, 2, cl, lab.data_ptr(), y.data_ptr(), None, None) == E_INVALID      # prob without prob_raw
    torch.cuda.synchronize()
    assert bool((lab == 77).all())
    with pytest.raises(lib.Met2Error):
        motor.tissue_segment_filter(np.ones((4, 4, 4)), n_class=9)
    with pytest.raises(lib.Met2Error):
        motor.tissue_segment_filter(np.ones((4, 4, 4)), beta=-1.0)
    with pytest.raises(ValueError):
        motor.tissue_segment_filter(np.ones((4, 4)))
    with pytest.raises(ValueError):
        motor.tissue_segment_filter(np.ones((4, 4, 4)), np.ones((4, 4, 3)))
    with pytest.raises(ValueError):
        motor.tissue_segment_filter(np.ones((4, 4, 4)), voxel_size=(1.0, 1.0))


def driver_volume():
    """16 x 16 x 8 x 32: a two-pool decay whose amplitude follows a smooth field, three tissue levels, 1 % noise; the mask leaves a rim out"""
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


def test_drivers_take_segment(motor, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    data, mask, TE = driver_volume()
    args = (mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    vox = (2.0, 2.5, 4.0)
    no = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="no")
    assert "TWC_seg" not in no and "TWC_prob" not in no
    s, p, _ = motor.tissue_segment_filter(no["TWC"], mask, vox)
    assert len(np.unique(s)) == 4
    for kw in ({}, {"devices": [0]}):
        got = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="yes", **kw)
        assert sorted(got) == sorted(list(no) + ["TWC_seg", "TWC_prob"])
        for k in no:
            assert np.array_equal(got[k], no[k], equal_nan=True), (k, kw)
        assert got["TWC_seg"].dtype == np.uint8 and np.array_equal(got["TWC_seg"], s) and np.array_equal(got["TWC_prob"], p), kw
    # the on-disk driver
    aff = np.diag([2.0, -2.5, 4.0, 1.0])
    nifti.save(nifti.NiftiImage(data, aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(mask.astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/seg_"
    motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force", "no",
                           40.0, bias_correct="yes", segment="yes")
    on_disk = nifti.load(out + "TWC_seg.nii.gz").get_fdata()
    assert np.array_equal(on_disk, s)
    for k in range(3):
        assert np.array_equal(nifti.load(out + "TWC_prob_%d.nii.gz" % k).get_fdata(), p[k])
    assert not os.path.exists(out + "TWC_prob_3.nii.gz") and not os.path.exists(out + "TWC_pve_0.nii.gz")
    with pytest.raises(ValueError, match="needs bias_correct"):
        motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force",
                               "no", 40.0, segment="yes")
