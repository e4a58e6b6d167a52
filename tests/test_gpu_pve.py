"""GPU tests of met2_partial_volume and its stage entries (csrc/met2_pve.hip), motor.partial_volume_filter and segment='pve' in the drivers,
against the numpy restatement of the algorithm (tests/tools/pve_numpy.py, which follows include/met2_hip.h step by step).

Stages.  Moments: the chunks' partial sums equal to the bit to the same terms added on the host in the kernels' order (seg.chunk_sums); mu,
var, pi within 1e-12 relative of the long-double restatement.  Constants: within 4 ulp of numpy on the device's own moments (one division, or
the device's log against numpy's).  Energies, given the device's constants: the pure ones equal numpy's to the bit (every operation rounds
once on both sides); the mixed ones go through 128 exp and a log, so they are compared with the long-double restatement and may deviate 100
times as far as the fp64 restatement itself does on the same input (the margin tests/test_gpu_bet.py gives its vertices); +inf exactly on the
dead types.  ICM, given E: the types are discrete, so EQUAL types in every voxel after each colour pass and after 8 sweeps.  Finish: pve
within 1e-12, pveseg and mixeltype equal.
Shapes: the tile of pve_icm_kernel is 4 x 8 x 16 voxels; 1 x 1 x 1, 3 x 1 x 40, one tile, one voxel past a seam and past two seams on
every axis; domains of 1023 / 1024 / 1025 / 2049 voxels (the chunks of the sums are 1024 list entries) picked at random, so full of holes.

Whole filter, fed the segmentation restatement's seg and prob.  mixeltype and pveseg equal in every voxel, pve within 1e-9 absolute,
classes_lin within 1e-9 relative of the long-double restatement.  What allows equal types is a condition the test asserts on the CPU first:
the long-double restatement's smallest relative gap between the two lowest energies, over every visit of every sweep, is >= 1e-9.
Measured figures: profiles/pve_parity.json."""
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
import pve_numpy as pn                                             # noqa: E402
import seg_numpy as sn                                             # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
TILE = (4, 8, 16)                                                  # pve_icm_kernel's tile (x, y, z)
BETA_PV, N_ICM = 0.3, 8
LD = np.longdouble


def record(name, figures):
    """with MET2_PVE_PARITY_JSON set, the measured deviations are kept in that file (profiles/pve_parity.json was written this way)"""
    path = os.environ.get("MET2_PVE_PARITY_JSON")
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
def pve(motor):
    return importlib.import_module(PKG + ".pve")


def ulps(x, ref):
    """the largest |x - ref| in units of ref's spacing; an entry whose reference is 0 must be 0"""
    x, ref = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    zero = ref == 0
    assert np.all(x[zero] == 0.0)
    if zero.all():
        return 0.0
    return float((np.abs(x - ref)[~zero] / np.spacing(np.abs(ref[~zero]))).max())


def test_the_shapes_cross_the_seams(pve):
    assert pve.TILE == TILE == pn.TILE and pve.CHUNK == pn.CHUNK == 1024 and pve.N_NODES == pn.N_NODES
    shapes = [c[0] for c in pn.CASES.values()]
    for want in ((1, 1, 1), (3, 1, 40), (4, 8, 16), (5, 9, 17), (9, 17, 33)):
        assert want in shapes
    assert (5, 9, 17) == tuple(t + 1 for t in TILE) and (9, 17, 33) == tuple(2 * t + 1 for t in TILE)
    sizes = [int(pn.case(n)["om"].sum()) for n in pn.CASES]
    for want in (1023, 1024, 1025, 2049):
        assert want in sizes
    assert sorted({c[2] for c in pn.CASES.values()}) == [1, 2, 3, 8]
    assert any(len(set(c[1])) == 3 for c in pn.CASES.values())           # an anisotropic voxel
    assert any(c[5] is not None for c in pn.CASES.values())              # a dead class


@functools.lru_cache(maxsize=None)
def device_stage(name):
    """what the device's first stages give for a case, computed once and never written to: classes (mu, var, pi), the constants, E and the
    first types"""
    pve = importlib.import_module(PKG + ".pve")
    c = pn.case(name)
    mo = pve.pve_moments(c["v"], c["seg"], c["prob"])
    a, h, live, tab = pve.pve_consts(mo["classes"])
    E, t0 = pve.pve_energy(c["v"], c["seg"], mo["classes"])
    out = {"mo": mo, "classes": mo["classes"], "mu": mo["classes"][:c["K"]], "a": a, "h": h, "live": live, "tab": tab, "E": E, "t0": t0,
           "w": sn.axis_weights(c["voxel"])}
    for x in list(out.values()) + list(mo.values()):
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return out


@pytest.mark.parametrize("name", pn.CASES)
def test_moments(pve, name):
    c, d = pn.case(name), device_stage(name)
    K, mo = c["K"], d["mo"]
    N = int(c["om"].sum())
    assert mo["n_domain"] == N
    mu, var, pi = (mo["classes"][i * K:(i + 1) * K] for i in range(3))
    u = c["v"][c["om"]]
    p = c["prob"][:, c["om"]]
    dd = u[None, :] - mu[:, None]                                        # the device's own means
    terms = np.stack([p, p * u[None, :], (p * dd) * dd])
    part = pve.chunk_sums(terms)
    assert mo["part"].shape == part.shape == (3, K, -(-N // 1024))
    assert np.array_equal(mo["part"], part)
    assert np.array_equal(mo["sums"], pve.partial_sum(part))
    ref = pn.moments(c["v"], c["seg"], c["prob"], LD)
    refc = np.concatenate([ref["mu"], ref["var"], ref["pi"]])
    nz = refc != 0
    assert np.array_equal(mo["classes"] == 0, ~nz)
    e = float(np.abs(mo["classes"][nz] / refc[nz] - 1.0).max()) if nz.any() else 0.0
    print("%s: N = %d, moments within %.3e relative of long double" % (name, N, e))
    record("moments_" + name, {"shape": list(c["v"].shape), "n_domain": N, "classes_rel": e})
    assert e <= 1e-12
    if c["dead"] is None:
        assert abs(float(pi.sum()) - 1.0) <= 1e-12                       # the posteriors of a voxel sum to 1


@pytest.mark.parametrize("name", pn.CASES)
def test_consts(pve, name):
    c, d = pn.case(name), device_stage(name)
    K = c["K"]
    mu, var, pi = (d["classes"][i * K:(i + 1) * K] for i in range(3))
    a, h, live, tab = pn.consts(mu, var, pi)
    assert d["live"].dtype == bool and np.array_equal(d["live"], live)
    figs = {"a_ulp": ulps(d["a"], a), "h_ulp": ulps(d["h"], h), "m_ulp": ulps(d["tab"][..., 0], tab[..., 0]),
            "a_jm_ulp": ulps(d["tab"][..., 1], tab[..., 1]), "h_jm_ulp": ulps(d["tab"][..., 2], tab[..., 2])}
    print(name, figs)
    record("consts_" + name, figs)
    assert d["tab"].shape == (K - 1, 64, 3) and max(figs.values()) <= 4.0


def test_consts_of_dead_classes(pve):
    mu, var, pi = np.array([500.0, 800.0, 1100.0]), np.array([400.0, 900.0, 1600.0]), np.array([0.3, 0.3, 0.4])
    rows = [(mu, var, pi), (mu, var, np.array([0.3, 0.0, 0.7])), (np.array([500.0, 500.0, 1100.0]), var, pi), (mu[::-1].copy(), var, pi)]
    rows += [(mu, np.array([400.0, 900.0, bad]), pi) for bad in (0.0, -1.0, np.nan, np.inf)]
    for m, v, p in rows:
        a, h, live, tab = pve.pve_consts(np.concatenate([m, v, p]))
        ra, rh, rlive, rtab = pn.consts(m, v, p)
        assert np.array_equal(live, rlive), (m, v, p)
        assert ulps(a, ra) <= 4 and ulps(h, rh) <= 4 and ulps(tab, rtab) <= 4
    assert pve.pve_consts(np.concatenate([mu, var, np.zeros(3)]))[2].tolist() == [False] * 5


@pytest.mark.parametrize("name", pn.CASES)
def test_energies(pve, name):
    c, d = pn.case(name), device_stage(name)
    K, om, E = c["K"], c["om"], d["E"]
    assert E.shape == (2 * K - 1,) + c["v"].shape and E.dtype == np.float64
    args = (d["mu"], d["a"], d["h"], d["live"], d["tab"])                # the device's constants go to the restatement
    r64 = pn.energies(c["v"], om, *args)
    r80 = pn.energies(c["v"].astype(LD), om, *[x.astype(LD) if x.dtype != bool else x for x in args])
    assert np.array_equal(E[:K], r64[:K])                                # pure: to the bit (+inf on a dead class included)
    assert np.all(E[:, ~om] == 0.0)
    for t in range(2 * K - 1):                                           # +inf exactly on the dead types
        assert np.all(np.isinf(E[t][om]) & (E[t][om] > 0)) if not d["live"][t] else np.all(np.isfinite(E[t][om]))
    mixed = np.zeros(E.shape, dtype=bool)
    mixed[K:] = om[None] & d["live"][K:][(slice(None),) + (None,) * 3]
    if mixed.any():
        own = float(np.abs(r64.astype(LD) - r80)[mixed].max())
        dev = float(np.abs(E.astype(LD) - r80)[mixed].max())
        print("%s: mixed energies up to %.1f: the device %.3e from long double, the fp64 restatement %.3e" % (
            name, float(np.abs(E[mixed]).max()), dev, own))
        record("energy_" + name, {"shape": list(c["v"].shape), "device_abs": dev, "fp64_restatement_abs": own,
                                  "largest_energy": float(np.abs(E[mixed]).max())})
        assert dev <= 100.0 * own
    t0 = d["t0"]
    assert t0.dtype == np.uint8 and np.array_equal(t0, pn.init_types(E, om, d["live"], c["seg"]))
    if not d["live"].any():
        assert np.array_equal(t0[om], c["seg"][om] - 1)


def where_differs(got, ref, start_gaps):
    """the assertion message when types differ: where, and the restatement's relative energy gap there"""
    bad = np.argwhere(got != ref)
    if len(bad) == 0:
        return ""
    i = tuple(bad[0])
    return "%d types differ, the first at %s: device %d, restatement %d, the restatement's smallest relative energy gap there %.3e (smallest over those %.3e)" % (
        len(bad), i, got[i], ref[i], start_gaps[i], min(start_gaps[tuple(b)] for b in bad))


@pytest.mark.parametrize("name", pn.CASES)
def test_icm_gives_the_restatements_types(pve, name):
    c, d = pn.case(name), device_stage(name)
    E, live, w, om = d["E"], d["live"], d["w"], c["om"]
    rng = np.random.default_rng(700 + sorted(pn.CASES).index(name))
    alive = np.flatnonzero(live)
    starts = [d["t0"]]
    if len(alive):                                                       # random live types: every voxel far from its optimum
        starts.append(np.where(om, alive[rng.integers(0, len(alive), size=om.shape)], pn.OFF).astype(np.uint8))
    for start in starts:
        gaps = np.full(om.shape, np.inf)
        r8 = pn.icm(start, E, live, w, BETA_PV, N_ICM, gaps=gaps)
        r0 = pn.icm_pass(start, E, live, w, BETA_PV, 0)
        r1 = pn.icm_pass(r0, E, live, w, BETA_PV, 1)
        p0 = pve.pve_icm(start, E, live, w, BETA_PV, 1, colour=0)
        assert p0.dtype == np.uint8 and np.array_equal(p0, r0), where_differs(p0, r0, gaps)
        colour = sn.colour_of(start.shape)
        assert np.array_equal(p0[colour == 1], start[colour == 1])       # the other colour is not touched
        p1 = pve.pve_icm(p0, E, live, w, BETA_PV, 1, colour=1)
        assert np.array_equal(p1, r1), where_differs(p1, r1, gaps)
        s1 = pve.pve_icm(start, E, live, w, BETA_PV, 1)
        assert np.array_equal(s1, r1), where_differs(s1, r1, gaps)
        s8 = pve.pve_icm(start, E, live, w, BETA_PV, N_ICM)
        assert np.array_equal(s8, r8), where_differs(s8, r8, gaps)
        assert np.array_equal(pve.pve_icm(start, E, live, w, BETA_PV, 0), start)
        assert np.all(s8[~om] == pn.OFF)
        if len(alive):
            assert np.all(live[s8[om]])
        print("%s: one sweep changes %.1f %% of the types, eight %.1f %%" % (name, 100 * float((s1 != start)[om].mean()),
                                                                           100 * float((s8 != start)[om].mean())))
    if c["dead"] is not None:
        assert not np.isin(s8[om], [c["dead"], c["K"] + c["dead"], c["K"] + c["dead"] - 1]).any()
    if not len(alive):
        assert np.array_equal(s8, d["t0"])                               # no live type: nothing moves


def test_icm_takes_tensors_and_leaves_its_input(pve):
    c, d = pn.case("tile+1"), device_stage("tile+1")
    Et = torch.as_tensor(d["E"], device="cuda")
    tt = torch.as_tensor(d["t0"], device="cuda")
    out = pve.pve_icm(tt, Et, d["live"], d["w"], BETA_PV, 2)
    assert torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8
    assert np.array_equal(tt.cpu().numpy(), d["t0"]) and np.array_equal(Et.cpu().numpy(), d["E"])
    assert np.array_equal(out.cpu().numpy(), pn.icm(d["t0"], d["E"], d["live"], d["w"], BETA_PV, 2))
    with pytest.raises(ValueError):
        pve.pve_icm(np.full(d["t0"].shape, 5, dtype=np.uint8), d["E"], d["live"])      # a type that is none
    with pytest.raises(ValueError):
        pve.pve_icm(d["t0"], d["E"], d["live"], colour=2)
    with pytest.raises(ValueError):
        pve.pve_icm(d["t0"], d["E"], d["live"][:3])


@pytest.mark.parametrize("name", pn.CASES)
def test_finish(pve, name):
    c, d = pn.case(name), device_stage(name)
    typ = pn.icm(d["t0"], d["E"], d["live"], d["w"], BETA_PV, 2)
    p, ps, mx = pve.pve_finish(c["v"], typ, d["classes"])
    rp, rps, rmx = pn.finish(c["v"], typ, d["mu"])
    e = float(np.abs(p - rp).max())
    print("%s: max |pve - ref| = %.3e" % (name, e))
    record("finish_" + name, {"pve_abs": e})
    assert p.shape == (c["K"],) + typ.shape and p.dtype == np.float64 and e <= 1e-12
    assert ps.dtype == np.uint8 and np.array_equal(ps, rps) and mx.dtype == np.uint8 and np.array_equal(mx, rmx) and np.array_equal(mx, typ)


# ---- the whole filter ----

@functools.lru_cache(maxsize=None)
def reference(name):
    """the long-double restatement of a case and its relative energy gaps per voxel: computed once, shared, never written to"""
    c = pn.case(name)
    ref = pn.partial_volume(c["v"], c["seg"], c["prob"], c["voxel"], BETA_PV, N_ICM, dtype=LD)
    gaps, typ = pn.energy_gap(ref["E"], ref["om"], ref["live"], c["seg"], ref["w"], BETA_PV, N_ICM)
    assert np.array_equal(typ, ref["mixeltype"])
    for a in list(ref.values()) + [gaps]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref, gaps


@pytest.mark.parametrize("name", pn.CASES)
def test_parity_with_the_restatement(motor, name):
    c = pn.case(name)
    ref, gaps = reference(name)
    K = c["K"]
    assert gaps.min() >= 1e-9                                            # the condition: no type of this case hangs on a rounding
    p, ps, mx, cl = motor.partial_volume_filter(c["v"], None, c["voxel"], n_class=K, seg=c["seg"], prob=c["prob"])
    assert p.shape == (K,) + c["v"].shape and p.dtype == np.float64 and cl.shape == (3 * K,)
    assert ps.dtype == np.uint8 and mx.dtype == np.uint8 and ps.shape == mx.shape == c["v"].shape
    e_pve = float(np.abs(p.astype(LD) - ref["pve"]).max())
    nz = ref["classes_lin"] != 0
    e_cls = float(np.abs(cl[nz] / ref["classes_lin"][nz] - 1.0).max()) if nz.any() else 0.0
    print("%s %s: %d types differ, smallest relative gap %.3e, max |pve - ref| = %.3e, classes %.3e" % (
        name, c["v"].shape, int((mx != ref["mixeltype"]).sum()), float(gaps.min()), e_pve, e_cls))
    record(name, {"shape": list(c["v"].shape), "n_domain": int(c["om"].sum()), "types_differ": int((mx != ref["mixeltype"]).sum()),
                  "smallest_relative_gap": float(gaps.min()) if np.isfinite(gaps.min()) else None, "pve_abs": e_pve, "classes_rel": e_cls})
    assert np.array_equal(mx, ref["mixeltype"]), where_differs(mx, ref["mixeltype"], gaps)
    assert np.array_equal(ps, ref["pveseg"])
    assert e_pve <= 1e-9
    assert e_cls <= 1e-9 and np.all(cl[~nz] == 0.0)
    om = c["om"]
    assert np.all(p >= 0.0) and np.all(p[:, ~om] == 0.0) and np.abs(p.sum(axis=0)[om] - 1.0).max() <= 2.0 ** -52
    assert np.all(ps[~om] == 0) and np.all(mx[~om] == pn.OFF)


def test_deterministic_and_independent_of_the_embedding(motor):
    c = pn.case("n2049")
    a = motor.partial_volume_filter(c["v"], None, c["voxel"], seg=c["seg"], prob=c["prob"])
    b = motor.partial_volume_filter(c["v"], None, c["voxel"], seg=c["seg"], prob=c["prob"])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # embedded at an even offset: the colours of the checkerboard are those of the absolute coordinates, so an odd offset swaps the two passes
    pad = ((1, 1), (1, 2), (2, 1))
    big_v = np.pad(c["v"], pad, constant_values=123.0)
    big_s = np.pad(c["seg"], pad, constant_values=0)
    big_p = np.pad(c["prob"], ((0, 0),) + pad, constant_values=0.0)
    p, ps, mx, cl = motor.partial_volume_filter(big_v, None, c["voxel"], seg=big_s, prob=big_p)
    inner = tuple(slice(lo, -hi) for lo, hi in pad)
    assert np.array_equal(p[(slice(None),) + inner], a[0]) and np.array_equal(ps[inner], a[1]) and np.array_equal(mx[inner], a[2])
    assert np.array_equal(cl, a[3])
    margin = np.ones(big_v.shape, dtype=bool)
    margin[inner] = False
    assert np.all(p[:, margin] == 0.0) and np.all(ps[margin] == 0) and np.all(mx[margin] == pn.OFF)      # nothing in the margin


def test_faces_null_outputs_and_degenerate_volumes(motor):
    c = pn.case("tile+1")
    v, seg, prob, vox = c["v"], c["seg"], c["prob"], c["voxel"]
    want_all = motor.partial_volume_filter(v, None, vox, seg=seg, prob=prob)
    t = motor.partial_volume_filter(torch.as_tensor(v, device="cuda"), None, vox, seg=torch.as_tensor(seg, device="cuda"),
                                    prob=torch.as_tensor(prob, device="cuda"))
    assert all(torch.is_tensor(x) and x.is_cuda for x in t)
    for x, y in zip(t, want_all):
        assert np.array_equal(x.cpu().numpy(), y)
    pkg = importlib.import_module(PKG)
    assert pkg.partial_volume_filter is motor.partial_volume_filter
    # without seg and prob the filter runs the segmentation itself
    s, pr, _ = motor.tissue_segment_filter(v, None, vox)
    own = motor.partial_volume_filter(v, None, vox)
    fed = motor.partial_volume_filter(v, None, vox, seg=s, prob=pr)
    for x, y in zip(own, fed):
        assert np.array_equal(x, y)
    L = importlib.import_module(PKG + "._lib").lib()
    dd, sg, pb = (torch.as_tensor(x, device="cuda").contiguous() for x in (v, seg, prob))
    vx = (ctypes.c_double * 3)(*vox)
    nx, ny, nz = dd.shape
    for want in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (False, False, False, False)):
        outs = [torch.full((3,) + tuple(dd.shape), 99.0, dtype=torch.float64, device="cuda"),
                torch.full(tuple(dd.shape), 99, dtype=torch.uint8, device="cuda"), torch.full(tuple(dd.shape), 99, dtype=torch.uint8, device="cuda"),
                torch.full((9,), 99.0, dtype=torch.float64, device="cuda")]
        assert L.met2_partial_volume(0, nx, ny, nz, dd.data_ptr(), sg.data_ptr(), pb.data_ptr(), vx, 3, BETA_PV, N_ICM,
                                     *[o.data_ptr() if w else None for o, w in zip(outs, want)], None) == 0
        for o, w, ref in zip(outs, want, want_all):
            assert np.array_equal(o.cpu().numpy(), ref) if w else bool((o == 99).all())
    # an empty domain, and n_icm = 0: the first types
    p, ps, mx, cl = motor.partial_volume_filter(v, None, vox, seg=np.zeros_like(seg), prob=np.zeros_like(prob))
    assert np.all(p == 0.0) and np.all(ps == 0) and np.all(mx == pn.OFF) and np.all(cl == 0.0)
    first = motor.partial_volume_filter(v, None, vox, n_icm=0, seg=seg, prob=prob)[2]
    assert np.array_equal(first, device_stage("tile+1")["t0"])
    # no class with weight: the fractions are the labels
    p, ps, mx, cl = motor.partial_volume_filter(v, None, vox, seg=seg, prob=np.zeros_like(prob))
    assert np.array_equal(ps, seg) and np.array_equal(mx, np.where(seg == 0, pn.OFF, seg - 1).astype(np.uint8))
    for k in range(3):
        assert np.array_equal(p[k], (seg == k + 1).astype(np.float64))


def test_return_codes(motor, pve):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    dd = torch.full((8, 8, 8), 5.0, dtype=torch.float64, device="cuda")
    sg = torch.ones((8, 8, 8), dtype=torch.uint8, device="cuda")
    pb = torch.full((8, 8, 8, 8), 0.125, dtype=torch.float64, device="cuda")     # room for K = 8
    po = torch.full((8, 8, 8, 8), 7.0, dtype=torch.float64, device="cuda")
    so = torch.full((8, 8, 8), 77, dtype=torch.uint8, device="cuda")
    mo = torch.full((8, 8, 8), 77, dtype=torch.uint8, device="cuda")
    co = torch.full((24,), 7.0, dtype=torch.float64, device="cuda")

    def call(nx=8, ny=8, nz=8, v=dd, seg=sg, prob=pb, vox=(2.0, 2.0, 2.0), K=3, beta_pv=0.3, n_icm=8):
        ptr = lambda x: None if x is None else x.data_ptr()
        return L.met2_partial_volume(0, nx, ny, nz, ptr(v), ptr(seg), ptr(prob), None if vox is None else (ctypes.c_double * 3)(*vox), K, beta_pv,
                                     n_icm, po.data_ptr(), so.data_ptr(), mo.data_ptr(), co.data_ptr(), None)

    assert call(v=None) == E_INVALID and call(seg=None) == E_INVALID and call(prob=None) == E_INVALID
    assert call(nx=-1) == E_INVALID and call(ny=-1) == E_INVALID and call(nz=-1) == E_INVALID
    assert call(K=0) == E_INVALID and call(n_icm=-1) == E_INVALID
    for bad in (-0.1, float("nan"), float("inf"), float("-inf")):
        assert call(beta_pv=bad) == E_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(vox=(bad, 2.0, 2.0)) == E_INVALID and call(vox=(2.0, 2.0, bad)) == E_INVALID
    assert call(vox=None) == E_INVALID
    assert call(K=9) == E_UNSUPPORTED
    assert call(nx=2048, ny=1024, nz=1024) == E_UNSUPPORTED            # 2^31 voxels; nothing is read
    for shape in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert call(*shape) == 0
    assert call(0, 8, 8, v=None) == 0
    assert call(0, 8, 8, K=0) == E_INVALID and call(0, 8, 8, beta_pv=-1.0) == E_INVALID
    # the stage entries
    y = torch.zeros(8, dtype=torch.float64, device="cuda")
    E5 = torch.zeros(40, dtype=torch.float64, device="cuda")
    lab = torch.full((8,), 77, dtype=torch.uint8, device="cuda")
    cl = (ctypes.c_double * 9)(500.0, 800.0, 1100.0, 100.0, 100.0, 100.0, 0.3, 0.3, 0.4)
    lv = (ctypes.c_int32 * 5)(1, 1, 1, 1, 1)
    w = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    yp, lp, ep = y.data_ptr(), lab.data_ptr(), E5.data_ptr()
    assert L.met2_pve_moments(0, 0, yp, lp, yp, 1, None, None, None, None) == E_INVALID
    assert L.met2_pve_moments(0, 8, None, lp, yp, 1, None, None, None, None) == E_INVALID
    assert L.met2_pve_moments(0, 8, yp, lp, yp, 0, None, None, None, None) == E_INVALID
    assert L.met2_pve_moments(0, 8, yp, lp, yp, 9, None, None, None, None) == E_UNSUPPORTED
    assert L.met2_pve_consts(0, 0, cl, None, None, None, None, None) == E_INVALID and L.met2_pve_consts(0, 9, cl, None, None, None, None, None) == E_UNSUPPORTED
    assert L.met2_pve_consts(0, 3, None, None, None, None, None, None) == E_INVALID
    assert L.met2_pve_energy(0, 0, yp, lp, 3, cl, ep, lp, None) == E_INVALID and L.met2_pve_energy(0, 8, yp, lp, 3, cl, None, lp, None) == E_INVALID
    assert L.met2_pve_energy(0, 8, yp, lp, 3, None, ep, lp, None) == E_INVALID
    assert L.met2_pve_icm(0, 2, 2, 0, lp, ep, 3, lv, w, 0.3, 1, -1, None) == E_INVALID
    assert L.met2_pve_icm(0, 2, 2, 2, lp, ep, 3, lv, w, -0.3, 1, -1, None) == E_INVALID
    assert L.met2_pve_icm(0, 2, 2, 2, lp, ep, 3, lv, w, 0.3, -1, -1, None) == E_INVALID
    assert L.met2_pve_icm(0, 2, 2, 2, lp, ep, 3, lv, w, 0.3, 1, 2, None) == E_INVALID
    assert L.met2_pve_icm(0, 2, 2, 2, lp, ep, 3, lv, None, 0.3, 1, -1, None) == E_INVALID
    assert L.met2_pve_icm(0, 2, 2, 2, lp, ep, 3, None, w, 0.3, 1, -1, None) == E_INVALID
    assert L.met2_pve_icm(0, 2, 2, 2, None, ep, 3, lv, w, 0.3, 1, -1, None) == E_INVALID
    assert L.met2_pve_finish(0, 8, yp, None, 3, cl, None, lp, None, None) == E_INVALID
    assert L.met2_pve_finish(0, 0, yp, lp, 3, cl, None, lp, None, None) == E_INVALID
    torch.cuda.synchronize()
    assert bool((so == 77).all()) and bool((mo == 77).all()) and bool((po == 7.0).all()) and bool((co == 7.0).all())      # nothing was launched
    assert bool((lab == 77).all()) and bool((E5 == 0.0).all())
    assert call(K=8) == 0 and call(n_icm=0) == 0 and call(beta_pv=0.0) == 0 and call(K=1) == 0
    assert bool((so == 1).all()) and bool((mo == 0).all())              # a constant volume: no class has a variance, the labels stand
    with pytest.raises(lib.Met2Error):
        motor.partial_volume_filter(np.ones((4, 4, 4)), n_class=9, seg=np.ones((4, 4, 4), dtype=np.uint8), prob=np.ones((9, 4, 4, 4)))
    with pytest.raises(lib.Met2Error):
        motor.partial_volume_filter(np.ones((4, 4, 4)), beta_pv=-1.0, seg=np.ones((4, 4, 4), dtype=np.uint8), prob=np.ones((3, 4, 4, 4)))
    with pytest.raises(ValueError):
        motor.partial_volume_filter(np.ones((4, 4)), seg=np.ones((4, 4), dtype=np.uint8), prob=np.ones((3, 4, 4)))
    with pytest.raises(ValueError):
        motor.partial_volume_filter(np.ones((4, 4, 4)), seg=np.ones((4, 4, 3), dtype=np.uint8), prob=np.ones((3, 4, 4, 4)))
    with pytest.raises(ValueError):
        motor.partial_volume_filter(np.ones((4, 4, 4)), seg=np.ones((4, 4, 4), dtype=np.uint8), prob=np.ones((2, 4, 4, 4)))
    with pytest.raises(ValueError):
        motor.partial_volume_filter(np.ones((4, 4, 4)), voxel_size=(1.0, 1.0), seg=np.ones((4, 4, 4), dtype=np.uint8), prob=np.ones((3, 4, 4, 4)))


def driver_volume():
    """16 x 16 x 8 x 32: a two-pool decay whose amplitude follows a smooth field, three tissue levels, 1 % noise; the mask leaves a rim out
    (the volume of tests/test_gpu_seg.py)"""
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


def test_drivers_take_segment_pve(motor, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    data, mask, TE = driver_volume()
    args = (mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    vox = (2.0, 2.5, 4.0)
    new = ["TWC_pve", "TWC_pveseg", "TWC_mixeltype"]
    yes = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="yes")
    assert not any(k in yes for k in new)
    s, p, _ = motor.tissue_segment_filter(yes["TWC"], mask, vox)
    assert np.array_equal(yes["TWC_seg"], s) and np.array_equal(yes["TWC_prob"], p)      # 'yes' gives what it gave
    pv, ps, mx, _ = motor.partial_volume_filter(yes["TWC"], None, vox, seg=s, prob=p)
    assert np.array_equal(mx != pn.OFF, s > 0) and mx[s > 0].max() < 5 and np.abs(pv.sum(axis=0)[s > 0] - 1.0).max() <= 2.0 ** -52
    for kw in ({}, {"devices": [0]}):
        got = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="pve", **kw)
        assert sorted(got) == sorted(list(yes) + new)
        for k in yes:
            assert np.array_equal(got[k], yes[k], equal_nan=True), (k, kw)
        assert got["TWC_pve"].shape == (3,) + mask.shape and np.array_equal(got["TWC_pve"], pv), kw
        assert got["TWC_pveseg"].dtype == np.uint8 and np.array_equal(got["TWC_pveseg"], ps), kw
        assert got["TWC_mixeltype"].dtype == np.uint8 and np.array_equal(got["TWC_mixeltype"], mx), kw
    # the on-disk driver
    aff = np.diag([2.0, -2.5, 4.0, 1.0])
    nifti.save(nifti.NiftiImage(data, aff), str(tmp_path / "data.nii.gz"))
    nifti.save(nifti.NiftiImage(mask.astype(np.uint8), aff), str(tmp_path / "mask.nii.gz"))
    out = str(tmp_path) + "/pve_"
    motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force", "no",
                           40.0, bias_correct="yes", segment="pve")
    assert np.array_equal(nifti.load(out + "TWC_seg.nii.gz").get_fdata(), s)
    for k in range(3):
        assert np.array_equal(nifti.load(out + "TWC_prob_%d.nii.gz" % k).get_fdata(), p[k])
        assert np.array_equal(nifti.load(out + "TWC_pve_%d.nii.gz" % k).get_fdata(), pv[k])
    assert np.array_equal(nifti.load(out + "TWC_pveseg.nii.gz").get_fdata(), ps)
    assert np.array_equal(nifti.load(out + "TWC_mixeltype.nii.gz").get_fdata(), mx)
    assert not os.path.exists(out + "TWC_pve_3.nii.gz")
    with pytest.raises(ValueError, match="needs bias_correct"):
        motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "mask.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force",
                               "no", 40.0, segment="pve")
