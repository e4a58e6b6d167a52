"""The mutual-information costs of the registration (cost='mi' | 'nmi') without a device: the numpy restatement
(tests/tools/register_mi_numpy.py, the yardstick of tests/test_gpu_register_mi.py) against a case worked by hand and against the properties
of the measures, the worst values, the refusals of met2_register_joint_cost before any device work and its work space against the header's
formula, the rule that sizes the joint histogram per pyramid level, and the search itself, driven by the restatement as cost_fn, on the
remapped 20 x 18 x 16 phantom: a known transform is recovered to under half a fixed voxel (1 mm) by both measures at 6 and 12 degrees of
freedom -- and is NOT with 64 x 64 cells forced on every level, the case the rule is there for."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import register_mi_numpy as mn                                     # noqa: E402
import register_numpy as gn                                        # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"
HALF_VOXEL_MM = gn.PHANTOM_MM / 2.0
IDENTITY = np.eye(4)[:3]


@pytest.fixture(scope="module")
def reg():
    return importlib.import_module(PKG + ".register")


def test_restatement_by_hand():
    """12 voxels, 2 x 3 bins, counts [[3, 3, 0], [0, 0, 6]]: the moving bin determines the fixed one, so MI = Hx = log 2;
    Hy = Hxy = (3 / 2) log 2, so NMI = (Hx + Hy) / Hxy = 5 / 3"""
    fixed_bin = np.array([0] * 6 + [1] * 6, dtype=np.int32).reshape(2, 3, 2)
    moving = np.array([0.0] * 3 + [1.5] * 3 + [3.0] * 2 + [2.5] * 4).reshape(2, 3, 2)       # range (0, 3), scale 1: bins 0, 1, 2 (3.0 by the clamp)
    for kind, want in (("mi", -np.log(2.0)), ("nmi", -5.0 / 3.0)):
        n, c, joint = mn.prepare(None, fixed_bin, moving, kind, 2, 0.25, moving_bins=3)(IDENTITY, want_joint=True)
        assert n[0] == 12 and np.array_equal(joint[0], [[3, 3, 0], [0, 0, 6]]) and abs(c[0] - want) < 1e-15, kind
        assert abs(mn.prepare_fp64(None, fixed_bin, moving, kind, 2, 0.25, moving_bins=3)(IDENTITY)[1][0] - want) < 1e-14
    # the bin rule at its ends and edges, in fp64: lo and below in bin 0, hi and above in the last, an edge belongs to the bin above it
    assert list(mn.moving_bin(np.array([-1.0, 0.0, 0.999, 1.0, 2.0, 2.999, 3.0, 9.0]), (0.0, 3.0), 3)) == [0, 0, 0, 1, 2, 2, 2, 2]
    assert list(mn.moving_bin(np.array([2.0, 2.0]), (2.0, 2.0), 7)) == [0, 0]                 # hi = lo: bin 0
    # the entropies from the definition: a uniform row of four cells has log 4
    assert abs(mn.entropy([5, 5, 5, 5]) - np.log(np.longdouble(4))) < 1e-18 and mn.entropy([7]) == 0


def test_independent_and_identical_images():
    rng = np.random.default_rng(5)
    shape, B = (20, 20, 20), 4
    moving = rng.random(shape)
    fixed_bin = rng.integers(0, B, shape).astype(np.int32)
    # independent: the estimate's bias is about (B - 1)^2 / (2 N) = 5.6e-4 nats at N = 8000; ten times that is far from any dependence
    mi = mn.prepare(None, fixed_bin, moving, "mi", B, 0.25)(IDENTITY)[1][0]
    nmi = mn.prepare(None, fixed_bin, moving, "nmi", B, 0.25)(IDENTITY)[1][0]
    assert -5.6e-3 < mi <= 0.0 and -1.0 - 5.6e-3 < nmi <= -1.0
    # an image against itself: the histogram is diagonal, Hxy = Hx = Hy
    own = mn.moving_bin(moving, mn.range_of(moving), B).astype(np.int32)
    n, c, joint = mn.prepare(None, own, moving, "mi", B, 0.25)(IDENTITY, want_joint=True)
    assert n[0] == moving.size and np.array_equal(joint[0], np.diag(np.bincount(own.reshape(-1), minlength=B)))
    assert abs(c[0] + float(mn.entropy(np.bincount(own.reshape(-1))))) < 1e-15 and c[0] < -1.38          # close to log 4
    assert abs(mn.prepare(None, own, moving, "nmi", B, 0.25)(IDENTITY)[1][0] + 2.0) < 1e-15


def test_worst_values(reg):
    assert mn.worst("mi") == 0.0 and mn.worst("nmi") == -1.0
    rng = np.random.default_rng(6)
    shape = (9, 7, 5)
    moving, fixed_bin = rng.random(shape), rng.integers(0, 5, shape).astype(np.int32)
    outside = np.column_stack([np.eye(3), [-100.0, 0.0, 0.0]])
    half = np.column_stack([np.eye(3), [5.0, 0.0, 0.0]])           # 4 of the 9 planes stay inside
    for kind in mn.KINDS:
        w = mn.worst(kind)
        assert reg.worst(kind) == w
        f = mn.prepare(None, fixed_bin, moving, kind, 5, 0.25)
        assert f(outside)[0][0] == 0 and f(outside)[1][0] == w and f(IDENTITY)[1][0] < w
        assert mn.prepare(None, fixed_bin, np.full(shape, 3.7), kind, 5, 0.25)(IDENTITY)[1][0] == w       # one moving bin holds everything
        assert mn.prepare(None, fixed_bin, moving, kind, 5, 0.25, moving_bins=1)(IDENTITY)[1][0] == w
        assert mn.prepare(None, np.zeros(shape, dtype=np.int32), moving, kind, 1, 0.25, moving_bins=5)(IDENTITY)[1][0] == w   # one fixed bin
        n = mn.prepare(None, fixed_bin, moving, kind, 5, 0.0)(half)[0][0]
        assert n == 4 * 35
        assert mn.prepare(None, fixed_bin, moving, kind, 5, 0.45)(half)[1][0] == w                        # 140 of 315 inside: under 0.45 ...
        assert mn.prepare(None, fixed_bin, moving, kind, 5, 0.44)(half)[1][0] < w                         # ... and over 0.44
        assert np.isfinite(mn.prepare(None, np.full(shape, -1, dtype=np.int32), moving, kind, 5, 0.0)(IDENTITY)[1][0])   # nothing included
    assert reg.KINDS["mi"] == 3 and reg.KINDS["nmi"] == 4 and [reg.KINDS[k] for k in gn.KINDS] == [0, 1, 2]
    text = open(os.path.join(ROOT, "include", "met2_hip.h")).read()
    for line in ("#define MET2_REGISTER_MI 3", "#define MET2_REGISTER_NMI 4", "#define MET2_REGISTER_MI_WORST 0.0", "#define MET2_REGISTER_NMI_WORST -1.0"):
        assert line in text
    with pytest.raises(ValueError, match="corratio"):
        reg.worst("mutualinfo")


def test_ambiguous_names_the_samples_at_an_edge():
    fixed_bin = np.zeros((1, 1, 6), dtype=np.int32)
    fixed_bin[0, 0, 5] = -1
    y = np.array([0.0, 1.0, 1.0 + 1e-12, 1.5, 4.0, 2.0], dtype=np.longdouble).reshape(1, 1, 6)     # range (0, 4), 4 bins: scale 1
    ins = np.ones((1, 1, 6), dtype=bool)
    mask, edge = mn.ambiguous(fixed_bin, (0.0, 4.0), y, ins, 1, 4)
    # 0 and 4 are ends, not edges between two bins (the clamps decide there); 2.0 is at an edge but excluded
    assert list(mask.reshape(-1)) == [False, True, True, False, False, False] and list(edge.reshape(-1)[1:3]) == [1, 1]
    assert not mn.ambiguous(fixed_bin, (0.0, 4.0), y, ins, 1, 1)[0].any()


def test_the_library_refuses_before_any_device_work(reg):
    """as tests/test_register_host.py holds the existing entry: without a device the new entries answer MET2_E_INVALID (-1) or
    MET2_E_UNSUPPORTED (-2), never MET2_E_HIP; the pointers are never read"""
    _lib = importlib.import_module(PKG + "._lib")
    L = _lib.lib()
    for name in ("met2_register_joint_work_bytes", "met2_register_joint_cost"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.met2_abi_version() == 6
    i3 = lambda *d: (C.c_int32 * 3)(*d)
    r2 = lambda lo, hi: (C.c_double * 2)(lo, hi)
    A = np.ascontiguousarray(np.tile(np.eye(4)[:3], (3, 1, 1)))
    Ap = A.ctypes.data_as(_lib._dp)
    bad = A.copy()
    bad[2, 1, 3] = np.nan
    p, q, w, n, c, j = 4096, 8192, 16384, 32768, 65536, 131072          # stand-ins for device pointers: a refused call reads none of them
    need = reg.joint_work_bytes((3, 4, 5), 8, 6, 3)

    def cost(kind=3, fd=(3, 4, 5), bins=8, index=p, md=(4, 4, 4), moving=q, mr=r2(0, 1), mb=6, K=3, a=Ap, mo=0.25, work=w, wb=need, ni=n, co=c, jo=j):
        return L.met2_register_joint_cost(0, kind, i3(*fd), bins, index, i3(*md), moving, mr, mb, K, a, mo, work, wb, ni, co, jo, None)

    assert cost(kind=0) == -1 and cost(kind=2) == -1 and cost(kind=5) == -1 and cost(kind=-1) == -1
    assert cost(kind=4, fd=(3, 0, 5)) == -1 and cost(fd=(3, 4, 513)) == -2 and cost(md=(0, 4, 4)) == -1 and cost(md=(513, 4, 4)) == -2
    assert cost(bins=0) == -1 and cost(bins=257) == -2 and cost(K=0) == -1 and cost(K=257) == -2 and cost(mb=0) == -1 and cost(mb=257) == -2
    assert cost(index=None) == -1 and cost(moving=None) == -1 and cost(a=None) == -1 and cost(work=None) == -1 and cost(ni=None) == -1 and cost(co=None) == -1
    assert cost(mr=r2(1, 0)) == -1 and cost(mr=r2(0, np.inf)) == -1 and cost(mr=None) == -1
    assert cost(a=bad.ctypes.data_as(_lib._dp)) == -1
    assert cost(mo=-0.1) == -1 and cost(mo=1.1) == -1 and cost(mo=float("nan")) == -1
    assert cost(wb=need - 1) == -1 and str(need).encode() in L.met2_last_error()
    assert cost(work=w + 4) == -1 and cost(index=p + 2) == -1 and cost(jo=j + 2) == -1
    # the existing entry keeps refusing the new kinds
    assert L.met2_register_cost(0, 3, i3(3, 4, 5), 8, p, q, r2(0, 1), i3(4, 4, 4), q, r2(0, 1), 3, Ap, 0.25, w, 1 << 20, n, c, None) == -1
    assert L.met2_register_cost(0, 4, i3(3, 4, 5), 8, p, q, r2(0, 1), i3(4, 4, 4), q, r2(0, 1), 3, Ap, 0.25, w, 1 << 20, n, c, None) == -1


def test_joint_work_bytes(reg):
    """the header: work_bytes = 96 K + 4 K n_bins moving_bins"""
    assert reg.joint_work_bytes((9, 7, 5), 64, 64, 17) == 96 * 17 + 4 * 17 * 64 * 64
    assert reg.joint_work_bytes((128, 128, 64), 2, 3, 1) == 96 + 24
    assert reg.joint_work_bytes((1, 1, 1), 256, 256, 256) == 96 * 256 + 4 * 256 ** 3
    text = open(os.path.join(ROOT, "include", "met2_hip.h")).read()
    assert "work_bytes = 96 K + 4 K n_bins moving_bins" in text
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (257, 4, 1), (4, 257, 1), (4, 4, 257)):
        with pytest.raises(Exception):
            reg.joint_work_bytes((9, 7, 5), *bad)
    assert reg.work_bytes((9, 7, 5), 64, 17) == (4 * (2 * 65 + 315), 96 * 17 + 44 * 17 * (2 + 64))       # the existing figures stay


def test_level_rule(reg):
    """B = min(n_bins, max(4, integer cube root of n_included))"""
    assert [reg.level_bins(64, n) for n in (63, 64, 65)] == [4, 4, 4]                  # cube roots 3, 4, 4: the floor of 4 holds
    assert [reg.level_bins(64, n) for n in (124, 125, 126, 342, 343)] == [4, 5, 5, 6, 7]   # exact at the cubes
    assert reg.level_bins(64, 5760) == 17 and reg.level_bins(64, 10 ** 6) == 64 and reg.level_bins(256, 10 ** 6) == 100
    assert reg.level_bins(256, 10 ** 6 - 1) == 99 and reg.level_bins(256, 512 ** 3) == 256
    assert [reg.level_bins(2, n) for n in (0, 63, 5760, 10 ** 6)] == [2, 2, 2, 2]      # n_bins caps the floor too
    assert reg.level_bins(64, 0) == 4 and reg.level_bins(3, 100) == 3
    with pytest.raises(ValueError, match="n_bins"):
        reg.level_bins(0, 100)


def _recording(seen):
    def cost_fn(fixed, fixed_bin, moving, kind, n_bins, min_overlap):
        seen.append((kind, n_bins, int(np.max(fixed_bin)), int((np.asarray(fixed_bin) >= 0).sum())))
        return mn.prepare_fp64(fixed, fixed_bin, moving, kind, n_bins, min_overlap)
    return cost_fn


@pytest.mark.parametrize("name", list(mn.E2E_CASES))
def test_register_recovers_a_known_transform(reg, name):
    true_world, dof, kind, (fx, fa, mv, ma, mask) = mn.e2e_case(name, reg)
    before = gn.mean_displacement(np.eye(4), true_world, mask, fa)
    assert before > 3.0
    seen = []
    out = reg.register(fx, fa, mv, ma, dof=dof, cost=kind, cost_fn=_recording(seen), filters=gn.FILTERS)
    after = gn.mean_displacement(out["world"], true_world, mask, fa)
    print("%s: mean displacement %.3f mm before, %.4f mm after; cost %.5f; %d evaluations" %
          (name, before, after, out["cost"], sum(l["n_eval"] for l in out["levels"])))
    assert after < HALF_VOXEL_MM
    # the levels hold 100, 720 and 5 760 voxels: 4, 8 and 17 bins, handed to cost_fn as n_bins with a fixed_bin of as many bins
    assert seen == [(kind, 4, 3, 100), (kind, 8, 7, 720), (kind, 17, 16, 5760)]
    assert out["dof"] == dof and out["n_inside"] > 0.25 * fx.size and out["cost"] < (-0.5 if kind == "mi" else -1.2)
    assert [l["dof"] for l in out["levels"]] == ([6, 7, 9, 12, 12] if dof == 12 else [6, 6, 6])
    if dof == 6:                                                   # deterministic: the same call gives the same matrix, to the bit
        again = reg.register(fx, fa, mv, ma, dof=dof, cost=kind, cost_fn=mn.prepare_fp64, filters=gn.FILTERS)
        assert np.array_equal(again["world"], out["world"]) and [l["cost"] for l in again["levels"]] == [l["cost"] for l in out["levels"]]


def test_a_fixed_histogram_size_runs_off(reg):
    """64 x 64 cells on every level, the rule ignored: the coarsest levels (100 and 720 voxels) have far more cells than samples, and the
    search ends further from the truth than it started.  The per-level rule exists for this case."""
    true_world, dof, kind, (fx, fa, mv, ma, mask) = mn.e2e_case("rigid6_mi", reg)

    def forced(fixed, fixed_bin, moving, kind, n_bins, min_overlap):
        b = reg.bin_intensity(fixed, 64)
        b[np.asarray(fixed_bin) < 0] = -1
        return mn.prepare_fp64(fixed, b, moving, kind, 64, min_overlap)

    out = reg.register(fx, fa, mv, ma, dof=dof, cost=kind, cost_fn=forced, filters=gn.FILTERS)
    before, after = gn.mean_displacement(np.eye(4), true_world, mask, fa), gn.mean_displacement(out["world"], true_world, mask, fa)
    print("64 x 64 cells on every level: %.3f mm before, %.3f mm after" % (before, after))
    assert after > before


def test_the_option_passes_through_the_filters(reg):
    filters = importlib.import_module(PKG + ".filters")
    true_world, dof, kind, (fx, fa, mv, ma, mask) = mn.e2e_case("rigid6_nmi", reg)
    opts = dict(dof=6, cost="nmi", scales_mm=[8.0, 4.0], max_sweeps=1, cost_fn=mn.prepare_fp64, filters=gn.FILTERS)
    world = filters.register_filter(fx, fa, mv, ma, **opts)
    assert np.array_equal(world, reg.register(fx, fa, mv, ma, **opts)["world"])
    assert gn.mean_displacement(world, true_world, mask, fa) < gn.PHANTOM_MM                 # levels down to 4 mm only: within a fixed voxel
    res = {"MWF": fx, "TWC": fx}
    with pytest.raises(ValueError, match="corratio"):                                       # the option reaches register's own check
        filters.atlas_stats_filter(res, gn.atlas_labels(), ma, fa, template=mv, register={"cost": "mutualinfo", "cost_fn": mn.prepare_fp64, "filters": gn.FILTERS})
