"""The numpy restatement of the brain extraction (tests/tools/bet_numpy.py, the reference of tests/test_gpu_bet.py) and its test volumes,
checked on the CPU so that the GPU tests cannot hide behind them: a known answer on the phantom, how far rounding moves the surface (the
figure the GPU tests' vertex bound is 100 times of), the mesh builders (the restatement's and the library's host one, which needs no GPU),
the fill against an analytic sphere and on the edge rule, the drivers' argument checks."""
import functools
import importlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bet_numpy as bn                                             # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"


@functools.lru_cache(maxsize=None)
def run(name, dtype="float64"):
    v, lab, vox, kw = bn.case(name)
    return bn.brain_mask(v, vox, dtype=np.dtype(dtype).type, **kw)


@pytest.mark.parametrize("name", list(bn.CASES))
def test_known_answer_on_the_phantom(name):
    """Dice against the phantom's true brain, measured with this restatement: 0.9746 ('small', level 3 x 300), 0.9780 ('aniso', level 3 x 200),
    0.9852 ('default': 64 x 72 x 56 voxels of 3 mm, level 4 x 1000, f = 0.4); no mask voxel in the scalp; the surface stops in the dark gap."""
    v, lab, vox, kw = bn.case(name)
    mask = run(name)["mask"].astype(bool)
    brain = lab == 1
    dice = 2.0 * (mask & brain).sum() / (mask.sum() + brain.sum())
    print(name, "dice %.4f, mask voxels in the gap %d, in the scalp %d, outside %d" % (dice, (mask & (lab == 2)).sum(), (mask & (lab == 3)).sum(),
                                                                                     (mask & (lab == 0)).sum()))
    assert dice >= 0.95
    assert not (mask & (lab == 3)).any() and not (mask & (lab == 0)).any()


@pytest.mark.parametrize("name", ["small", "aniso"])
def test_rounding_does_not_move_the_mask(name):
    """fp64 against long double through the whole filter: identical masks; the vertices differ by 6.3e-13 mm ('small') and 6.0e-13 mm ('aniso')
    (1.4e-12 mm on 'default', which takes half a minute in long double and is not run here)."""
    a, b = run(name), run(name, "longdouble")
    dev = float(np.abs(a["vertices"] - b["vertices"]).max())
    print(name, "max |vertex - long double| = %.3e mm" % dev)
    assert np.array_equal(a["mask"], b["mask"])
    assert dev <= 1e-9
    for k in bn.STAT_KEYS:
        assert abs(a["stats"][k] - b["stats"][k]) <= 1e-12 * abs(a["stats"][k]), k
    assert a["stats"]["count"] == b["stats"]["count"] and a["stats"]["n_tm"] == b["stats"]["n_tm"]


@pytest.mark.parametrize("name", list(bn.EVOLVE_CASES))
def test_evolve_cases_are_fit(name):
    """The deviation of the fp64 from the long-double evolution per committed case: what tests/test_gpu_bet.py multiplies by 100.  A case where
    a nearest-voxel sample lands on a rounding boundary shows as a deviation of the order of a voxel and is unfit: its seed or start has to
    change, not the bound.  Measured: at most 3.1e-13 mm on the ordinary cases, 4.2e-11 mm on 'flat' (every search leaves the volume),
    see the printed figures."""
    v, vox, st, level, n_iter, X0 = bn.evolve_case(name)
    ref, dev = bn.evolve_reference(name)
    print(name, "level %d, %d iterations: max |fp64 - long double| = %.3e mm (r = %.2f mm)" % (level, n_iter, dev, st["r"]))
    assert ref.shape == X0.shape and np.all(np.isfinite(ref))
    assert dev <= 1e-9
    if n_iter == 0:
        assert np.array_equal(ref, X0)
    else:
        assert np.abs(ref - X0).max() > 1e-3                             # the surface moved


def test_evolve_cases_are_what_they_say():
    levels = {bn.EVOLVE_CASES[k][1] for k in bn.EVOLVE_CASES}
    iters = {bn.EVOLVE_CASES[k][2] for k in bn.EVOLVE_CASES}
    assert {0, 1, 3, 4} <= levels and {0, 1, 49, 50, 51} <= iters
    assert bn.evolve_volume("aniso")[1] == (3.0, 3.0, 5.0) and bn.evolve_volume("mm1")[1] == (1.0, 1.0, 1.0)
    v, vox, st = bn.evolve_volume("flat")
    assert (v.shape[2] - 1) * vox[2] < 20.0
    v, vox, st, level, n_iter, X0 = bn.evolve_case("outside_l3_n51")
    ext = (np.array(v.shape) - 1) * np.array(vox)
    out = np.any((X0 < 0) | (X0 > ext), axis=1)
    assert 0.1 < out.mean() < 0.9                                        # the start sphere is partly outside the volume
    assert bn.icosphere(4)[0].shape[0] > 1024 and bn.icosphere(4)[0].shape[0] % 64 != 0


def mesh_is_sound(unit, tris, ring, deg, level):
    nv, nt = 10 * 4 ** level + 2, 20 * 4 ** level
    assert unit.shape == (nv, 3) and tris.shape == (nt, 3) and ring.shape == (nv, 6) and deg.shape == (nv,)
    assert np.abs(np.sqrt((unit ** 2).sum(axis=1)) - 1.0).max() < 1e-15
    assert set(np.unique(deg)) <= {5, 6} and int((deg == 5).sum()) == 12 and np.all(deg[:12] == 5)
    edges = {(min(a, b), max(a, b)) for t in tris for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    assert nv - len(edges) + nt == 2                                     # Euler characteristic
    directed = {(a, b) for t in tris for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    assert len(directed) == 3 * nt and all((b, a) in directed for a, b in directed)      # closed and consistently oriented
    tri_set = {tuple(int(x) for x in np.roll(t, -s)) for t in tris for s in range(3)}
    for i in range(nv):
        r = [int(x) for x in ring[i, :deg[i]]]
        assert np.all(ring[i, deg[i]:] == -1) and len(set(r)) == deg[i] and r[0] == min(r)
        for k in range(len(r)):                                          # every consecutive pair closes a triangle of the mesh, in its orientation
            assert (i, r[k], r[(k + 1) % len(r)]) in tri_set
    # outward: the triangle's normal points away from the origin
    a, b, c = unit[tris[:, 0]], unit[tris[:, 1]], unit[tris[:, 2]]
    assert np.all((np.cross(b - a, c - a) * (a + b + c)).sum(axis=1) > 0)


@pytest.mark.parametrize("level", range(5))
def test_mesh_builders(level):
    """the restatement's builder and the library's host one (met2_bet_mesh, no GPU needed) give the same mesh, bit for bit"""
    mesh = bn.icosphere(level)
    mesh_is_sound(*mesh, level)
    importlib.import_module(PKG + "._build").build()
    bet = importlib.import_module(PKG + ".bet")
    for a, b in zip(bet.bet_mesh(level), mesh):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    if level == 0:
        lib = importlib.import_module(PKG + "._lib")
        assert lib.lib().met2_bet_mesh(5, None, None, None, None) == -2 and lib.lib().met2_bet_mesh(-1, None, None, None, None) == -1


def test_library_exports_the_entries_as_the_header_declares_them():
    importlib.import_module(PKG + "._build").build()
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    assert L.met2_abi_version() == 6
    with open(os.path.join(ROOT, "include", "met2_hip.h")) as f:
        text = f.read()
    for name, nargs in (("met2_brain_mask", 13), ("met2_bet_mean", 6), ("met2_bet_stats", 9), ("met2_bet_mesh", 5), ("met2_bet_evolve", 13),
                        ("met2_bet_fill", 11)):
        assert name in lib.SYMBOLS and hasattr(L, name)
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m and len(m.group(1).split(",")) == nargs == len(getattr(L, name).argtypes), name


def test_fill_against_an_analytic_sphere():
    X, tris, shape, vox = bn.fill_case("sphere")
    mask, cross = bn.fill(X, tris, shape, vox, return_crossings=True)
    g = np.meshgrid(*[np.arange(n) * d for n, d in zip(shape, vox)], indexing="ij")
    rad = np.sqrt(sum((x - c) ** 2 for x, c in zip(g, (15.2, 14.9, 16.1))))
    # the level-2 mesh lies between its inscribed sphere (0.973 of the radius at the flattest face) and the sphere itself
    assert np.all(mask[rad <= 10.3 * 0.96] == 1) and np.all(mask[rad >= 10.3] == 0)
    assert abs(mask.sum() / (4.0 / 3.0 * np.pi * 10.3 ** 3) - 1.0) < 0.05
    assert np.all(cross % 2 == 0) and cross.max() == 2


@pytest.mark.parametrize("name", bn.FILL_CASES)
def test_fill_edge_rule(name):
    """every column has an even number of crossings, vertices and edges exactly on a column's line included"""
    X, tris, shape, vox = bn.fill_case(name)
    mask, cross = bn.fill(X, tris, shape, vox, return_crossings=True)
    print(name, shape, "inside", int(mask.sum()), "columns crossed", int((cross > 0).sum()))
    assert mask.shape == tuple(shape) and mask.dtype == np.uint8 and mask.any() and not mask.all()
    assert np.all(cross % 2 == 0)
    if name == "on_centre":
        assert X[0, 0] == 7 * vox[0] and X[0, 1] == 9 * vox[1]            # vertex 0 is on the line of column (7, 9)
    if name == "on_grid":
        assert np.all(X == np.round(X))                                  # every vertex on a column's line, edges along rows of columns
        # a permutation of the triangles or a rotation inside one changes nothing
        perm = np.roll(np.asarray(tris)[::-1], 1, axis=1)
        assert np.array_equal(bn.fill(X, perm, shape, vox), mask)
    # a column through the surface is filled between its two crossings only: the mask's columns are single runs on the convex meshes
    # (moving vertex 0 of 'on_centre' dents its mesh: up to four crossings there)
    runs = np.abs(np.diff(np.pad(mask.astype(np.int8), ((0, 0), (0, 0), (1, 1))), axis=2)).sum(axis=2)
    assert set(np.unique(runs)) <= ({0, 2, 4} if name == "on_centre" else {0, 2})


def test_stats_edge_conventions():
    rng = np.random.default_rng(5)
    v = rng.uniform(0.0, 1000.0, (10, 10, 10))                           # lo ~ 0, hi ~ 1000: bins of ~1
    st = st0 = bn.stats(v, (1.0, 2.0, 3.0))
    lo, hi = v.min(), v.max()
    s = np.sort(v.ravel())
    w = (hi - lo) / 1000.0
    assert abs(st["t2"] - s[19]) <= w and st["t2"] <= s[19]               # the lower edge of the bin that holds the 20th of 1000
    assert abs(st["t98"] - s[979]) <= w and st["t98"] >= s[979]           # the upper edge of the bin that holds the 980th
    assert st["t"] == st["t2"] + 0.1 * (st["t98"] - st["t2"])
    assert st["count"] == int((v > st["t"]).sum())
    assert abs(st["r"] - (3.0 * st["count"] * 6.0 / (4.0 * np.pi)) ** (1.0 / 3.0)) < 1e-12 * st["r"]
    # a constant volume with one voxel above it: the set is that voxel, the median's set is empty and tm = t
    c = np.full((6, 5, 4), 7.0)
    c[3, 2, 1] = 9.0
    st = bn.stats(c, (1.0, 1.0, 1.0))
    assert st["count"] == 1 and (st["cx"], st["cy"], st["cz"]) == (3.0, 2.0, 1.0) and st["n_tm"] == 0 and st["tm"] == st["t"]
    assert st["t2"] == 7.0 and st["t98"] == 7.0 + 2.0 / 1000.0
    with pytest.raises(ValueError):
        bn.stats(np.full((3, 3, 3), 2.0), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        bn.stats(np.full((3, 3, 3), np.nan), (1.0, 1.0, 1.0))
    # non-finite voxels are not there
    n = v.copy()
    n[0, 0, 0], n[1, 1, 1], n[2, 2, 2] = np.nan, np.inf, -np.inf
    a = bn.stats(n, (1.0, 2.0, 3.0))
    fin = np.isfinite(n)
    assert abs(a["t2"] - st0["t2"]) <= 3 * w and abs(a["t98"] - st0["t98"]) <= 3 * w and a["count"] == int((n[fin] > a["t"]).sum())
    m = bn.echo_mean(np.stack([v, n, v], axis=-1))
    assert np.array_equal(np.isfinite(m), np.isfinite(n)) and np.array_equal(m[np.isfinite(n)], ((v + n + v) / 3.0)[np.isfinite(n)])


def test_driver_argument_checks_raise_before_the_library_is_touched(monkeypatch):
    motor = importlib.import_module(PKG + ".motor")

    def no_lib():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(motor, "lib", no_lib)
    monkeypatch.setattr(importlib.import_module(PKG + ".bet"), "lib", no_lib)
    monkeypatch.setattr(importlib.import_module(PKG + ".filters"), "lib", no_lib)     # brain_mask_filter's
    data = np.ones((8, 8, 4, 32))
    mask = np.ones((8, 8, 4))
    TE = 10.0 * np.arange(1, 33)
    vox = (2.0, 2.0, 2.0)
    rec = lambda d, m, **kw: motor.recon_met2_arrays(d, m, TE, 3000.0, **kw)
    with pytest.raises(ValueError, match="brain_mask must be"):
        rec(data, mask, brain_mask="maybe")
    with pytest.raises(ValueError, match="does not go with a mask"):
        rec(data, mask, brain_mask="yes", voxel_size=vox)
    with pytest.raises(ValueError, match="prepared"):
        rec(data, None, brain_mask="yes", voxel_size=vox, prepared=True)
    with pytest.raises(ValueError, match="distributed"):
        rec(data, None, brain_mask="yes", voxel_size=vox, distributed=True)
    with pytest.raises(ValueError, match="voxel_size"):
        rec(data, None, brain_mask="yes")
    with pytest.raises(ValueError, match="voxel_size"):
        rec(data, None, brain_mask="yes", voxel_size=(1.0, 1.0))
    with pytest.raises(ValueError, match="nx,ny,nz,nt"):
        rec(data.reshape(-1, 32), None, brain_mask="yes", voxel_size=vox)
    with pytest.raises(ValueError, match="prepared"):                     # before degibbs runs anything
        rec(data, None, brain_mask="yes", voxel_size=vox, degibbs="yes", prepared=True)
    with pytest.raises(ValueError, match="nx,ny,nz"):
        motor.brain_mask_filter(np.ones((4, 4)), vox)
    with pytest.raises(ValueError, match="voxel_size"):
        motor.brain_mask_filter(np.ones((4, 4, 4)), (1.0, 1.0))
