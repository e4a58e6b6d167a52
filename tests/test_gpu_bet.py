"""GPU tests of met2_brain_mask and its stage entries (csrc/met2_bet.hip), motor.brain_mask_filter and brain_mask='yes' in the drivers,
against the numpy restatement of the algorithm (tests/tools/bet_numpy.py, which follows include/met2_hip.h step by step).

Tolerances.  Statistics: the thresholds t2, t, t98, the median tm, the centre of gravity and r within 1e-12 relative, the count of v > t
equal (the thresholds are defined operation by operation and come out bit-equal; the sums differ in their order of addition, 1e-16 sqrt N).
Evolution: max |vertex - restatement| <= max(100 x the restatement's own fp64-against-long-double deviation on that case, 1e-12 r):
tests/test_bet_host.py measures those deviations (at most 3.1e-13 mm, 4.2e-11 mm on 'flat') and shows that no committed case has a sample
on a rounding boundary.  Fill and the whole filter: the mask equal everywhere.

Shapes (bet_numpy.EVOLVE_CASES, FILL_CASES): mesh levels 0, 1, 3, 4 (2562 vertices: more than the workgroup's 1024 threads, no multiple of 64);
0, 1, 49, 50, 51 iterations (the seam of the refresh of l); voxels of (3, 3, 5) and (1, 1, 1) mm; an axis shorter than the 20 mm search; a
start sphere partly outside the volume; nx, ny, nz of 1, columns that are no multiple of the fill's workgroup, nz = 65; vertices and edges
exactly on a column's line."""
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
import bet_numpy as bn                                             # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
KEYS = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "fsol_4D", "Est_Signal", "reg_param")


def record(name, figures):
    """with MET2_BET_PARITY_JSON set, the measured deviations are kept in that file (profiles/bet_parity.json was written this way)"""
    path = os.environ.get("MET2_BET_PARITY_JSON")
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
def bet(motor):
    return importlib.import_module(PKG + ".bet")


@functools.lru_cache(maxsize=None)
def filter_reference(name):
    """the restatement's result on a committed case of the whole filter: computed once, shared, never written to"""
    v, lab, vox, kw = bn.case(name)
    res = bn.brain_mask(v, vox, **kw)
    res["mask"].setflags(write=False)
    res["vertices"].setflags(write=False)
    return v, vox, kw, res


def stats_volumes():
    rng = np.random.default_rng(11)
    v, vox, _ = bn.evolve_volume("aniso")                                # 45 x 41 x 23 = 42435 voxels: no multiple of the chunk of 1024
    holes = v.copy()
    holes[3, 4, 5], holes[20, 20, 10], holes[21, 20, 10], holes[44, 40, 22] = np.nan, np.inf, -np.inf, np.nan
    const = np.full((6, 5, 4), 7.0)
    const[3, 2, 1] = 9.0
    signed = rng.standard_normal((17, 9, 33)) * 50.0 + 20.0              # negative values: the keys of the median's selection change sign
    even = bn.evolve_volume("small")[0]
    return {"aniso": (v, vox), "holes": (holes, vox), "const_plus_one": (const, (1.0, 1.0, 1.0)), "signed": (signed, (0.7, 1.3, 2.1)),
            "small": (even, (3.0, 3.0, 3.0)), "one_chunk": (v[:10, :10, :10].copy(), (2.0, 2.0, 2.0))}


@pytest.mark.parametrize("name", ["aniso", "holes", "const_plus_one", "signed", "small", "one_chunk"])
def test_stats_against_the_restatement(bet, name):
    v, vox = stats_volumes()[name]
    ref = bn.stats(v, vox)
    got = bet.bet_stats(v, vox)
    rel = {k: abs(got[k] - ref[k]) / abs(ref[k]) if ref[k] != 0 else abs(got[k]) for k in bn.STAT_KEYS}
    print(name, v.shape, "count %d / %d, n_tm %d" % (got["count"], ref["count"], ref["n_tm"]), {k: "%.1e" % x for k, x in rel.items()})
    record("stats_" + name, {"shape": list(v.shape), "rel": rel})
    assert got["count"] == ref["count"]
    for k in bn.STAT_KEYS:
        assert rel[k] <= 1e-12, k
    again = bet.bet_stats(torch.as_tensor(v, device="cuda"), vox)
    assert again == got                                                  # bit for bit, and from a tensor
    if name == "const_plus_one":
        assert got["tm"] == got["t"] and (got["cx"], got["cy"], got["cz"]) == (3.0, 2.0, 1.0) and got["count"] == 1
    if name == "holes":
        assert not np.isfinite(v).all()


def test_echo_mean(bet):
    rng = np.random.default_rng(3)
    d = rng.uniform(0.0, 1000.0, (7, 5, 9, 32))
    d[1, 2, 3, 4], d[2, 2, 2, 0], d[3, 3, 3, 31] = np.nan, np.inf, -np.inf
    d[4, 4, 4, 1], d[4, 4, 4, 2] = np.inf, -np.inf
    got, ref = bet.bet_mean(d), bn.echo_mean(d)
    assert got.shape == (7, 5, 9) and np.array_equal(got, ref, equal_nan=True)
    assert np.isnan(got[1, 2, 3]) and got[2, 2, 2] == np.inf and got[3, 3, 3] == -np.inf and np.isnan(got[4, 4, 4])
    one = bet.bet_mean(d[..., :1])
    assert np.array_equal(one, d[..., 0], equal_nan=True)


@pytest.mark.parametrize("name", list(bn.EVOLVE_CASES))
def test_evolve_against_the_restatement(bet, name):
    v, vox, st, level, n_iter, X0 = bn.evolve_case(name)
    ref, dev = bn.evolve_reference(name)
    got = bet.bet_evolve(v, vox, st, X0, level, n_iter=n_iter)
    err = float(np.abs(got - ref).max())
    bound = max(100.0 * dev, 1e-12 * st["r"])
    print("%s: level %d, %d iterations, max |vertex - ref| = %.3e mm (bound %.3e; fp64 against long double %.3e)" % (name, level, n_iter, err, bound, dev))
    record("evolve_" + name, {"level": level, "n_iter": n_iter, "max_abs_mm": err, "bound_mm": bound, "fp64_vs_longdouble_mm": dev})
    assert got.shape == X0.shape and got.dtype == np.float64
    if n_iter == 0:
        assert np.array_equal(got, X0)
    assert err <= bound


def test_evolve_is_deterministic_and_works_in_place(bet):
    v, vox, st, level, n_iter, X0 = bn.evolve_case("l4_n51")
    a = bet.bet_evolve(v, vox, st, X0, level, n_iter=n_iter)
    b = bet.bet_evolve(torch.as_tensor(v, device="cuda"), vox, bn.stats_vector(st), torch.as_tensor(X0, device="cuda"), level, n_iter=n_iter)
    assert torch.is_tensor(b) and np.array_equal(b.cpu().numpy(), a)
    # 51 steps are 50 steps and one more only if l is refreshed at the 51st: the refresh belongs to the iteration's number, not to the call
    two = bet.bet_evolve(v, vox, st, bet.bet_evolve(v, vox, st, X0, level, n_iter=50), level, n_iter=1)
    assert np.array_equal(two, a)
    lib = importlib.import_module(PKG + "._lib").lib()
    x = torch.as_tensor(X0, device="cuda").clone()
    dd = torch.as_tensor(v, device="cuda")
    vx = (ctypes.c_double * 3)(*vox)
    sv = (ctypes.c_double * 8)(*bn.stats_vector(st))
    assert lib.met2_bet_evolve(0, *v.shape, dd.data_ptr(), vx, sv, 0.4, level, n_iter, x.data_ptr(), x.data_ptr(), None) == 0
    assert np.array_equal(x.cpu().numpy(), a)


@pytest.mark.parametrize("name", bn.FILL_CASES)
def test_fill_against_the_restatement(bet, name):
    X, tris, shape, vox = bn.fill_case(name)
    ref = bn.fill(X, tris, shape, vox)
    got = bet.bet_fill(X, tris, shape, vox)
    print(name, shape, "inside %d, differing %d" % (int(ref.sum()), int((got != ref).sum())))
    assert got.dtype == np.uint8 and got.shape == tuple(shape)
    assert np.array_equal(got, ref)
    t = bet.bet_fill(torch.as_tensor(X, device="cuda"), torch.as_tensor(np.asarray(tris), device="cuda"), shape, vox)
    assert torch.is_tensor(t) and np.array_equal(t.cpu().numpy(), ref)
    if name == "sphere":
        # a triangle that names a vertex that is not there is skipped; a mesh of none fills nothing
        bad = np.concatenate([np.asarray(tris), [[0, 1, X.shape[0]], [-1, 0, 1]]]).astype(np.int32)
        assert np.array_equal(bet.bet_fill(X, bad, shape, vox), ref)
        assert not bet.bet_fill(X, np.zeros((0, 3), dtype=np.int32), shape, vox).any()


@pytest.mark.parametrize("name", list(bn.CASES))
def test_filter_gives_the_restatements_mask(motor, name):
    v, vox, kw, ref = filter_reference(name)
    mask, verts, tris, st = motor.brain_mask_filter(v, vox, return_surface=True, **kw)
    err = float(np.abs(verts - ref["vertices"]).max())
    rel = max(abs(st[k] - ref["stats"][k]) / abs(ref["stats"][k]) for k in bn.STAT_KEYS)
    print("%s %s: %d voxels differ of %d inside, max |vertex - ref| = %.3e mm, statistics %.1e" % (name, v.shape, int((mask != ref["mask"]).sum()),
                                                                                                  int(ref["mask"].sum()), err, rel))
    record("filter_" + name, {"shape": list(v.shape), "mask_voxels_differing": int((mask != ref["mask"]).sum()), "vertices_max_abs_mm": err,
                              "stats_rel": rel, **kw})
    assert mask.dtype == np.uint8 and mask.shape == v.shape
    assert np.array_equal(tris, bn.icosphere(kw["level"])[1])
    assert rel <= 1e-12
    assert np.array_equal(mask, ref["mask"])


def test_filter_faces_4d_input_and_defaults(motor, bet):
    v, vox, kw, ref = filter_reference("small")
    plain = motor.brain_mask_filter(v, vox, **kw)
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, ref["mask"])
    t = motor.brain_mask_filter(torch.as_tensor(v, device="cuda"), vox, return_surface=True, **kw)
    assert torch.is_tensor(t[0]) and torch.is_tensor(t[1]) and np.array_equal(t[0].cpu().numpy(), plain)
    # 4-D data is averaged over the echoes first
    rng = np.random.default_rng(8)
    data = v[..., None] * np.exp(-np.arange(1, 5) / 3.0) * (1.0 + 0.01 * rng.standard_normal(v.shape + (4,)))
    mean = bet.bet_mean(data)
    assert np.array_equal(mean, bn.echo_mean(data))
    assert np.array_equal(motor.brain_mask_filter(data, vox, **kw), motor.brain_mask_filter(mean, vox, **kw))
    # the stages one after the other are the filter
    st = bet.bet_stats(v, vox)
    X = bet.bet_evolve(v, vox, st, bn.start_vertices(st, kw["level"]), kw["level"], kw["f"], kw["n_iter"])
    mask, verts, tris, st2 = motor.brain_mask_filter(v, vox, return_surface=True, **kw)
    assert {k: st[k] for k in bn.STAT_KEYS} == st2 and np.array_equal(verts, X)
    assert np.array_equal(bet.bet_fill(X, tris, v.shape, vox), mask)
    assert importlib.import_module(PKG).brain_mask_filter is motor.brain_mask_filter


def test_return_codes(motor):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    dd = torch.full((8, 8, 8), 5.0, dtype=torch.float64, device="cuda")
    dd[4, 4, 4] = 9.0
    m = torch.full((8, 8, 8), 7, dtype=torch.uint8, device="cuda")

    def call(nx=8, ny=8, nz=8, v=dd, vox=(2.0, 2.0, 2.0), f=0.4, level=1, n_iter=3, mask=m):
        return L.met2_brain_mask(0, nx, ny, nz, None if v is None else v.data_ptr(), None if vox is None else (ctypes.c_double * 3)(*vox), f, level,
                                 n_iter, None if mask is None else mask.data_ptr(), None, None, None)

    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert call(f=bad) == E_INVALID
    assert call(level=-1) == E_INVALID and call(level=5) == E_UNSUPPORTED
    assert call(n_iter=-1) == E_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(vox=(bad, 2.0, 2.0)) == E_INVALID and call(vox=(2.0, 2.0, bad)) == E_INVALID
    assert call(vox=None) == E_INVALID and call(v=None) == E_INVALID and call(mask=None) == E_INVALID
    assert call(nx=-1) == E_INVALID
    assert call(nx=2048, ny=1024, nz=1024) == E_UNSUPPORTED             # 2^31 voxels; nothing is read
    torch.cuda.synchronize()
    assert bool((m == 7).all())                                         # nothing was launched
    # an empty v > t set: a constant volume, no finite voxel, no voxel
    flat = torch.full((8, 8, 8), 5.0, dtype=torch.float64, device="cuda")
    assert call(v=flat) == E_INVALID and b"empty" in L.met2_last_error()
    assert call(v=torch.full((8, 8, 8), float("nan"), dtype=torch.float64, device="cuda")) == E_INVALID
    assert call(nx=0) == E_INVALID
    assert call() == 0 and call(level=0, n_iter=0) == 0 and call(level=4, n_iter=1) == 0
    # the stage entries share the checks
    st = (ctypes.c_double * 8)()
    vx = (ctypes.c_double * 3)(2.0, 2.0, 2.0)
    assert L.met2_bet_stats(0, 8, 8, 8, flat.data_ptr(), vx, st, None, None) == E_INVALID
    assert L.met2_bet_stats(0, 8, 8, 8, dd.data_ptr(), vx, None, None, None) == E_INVALID
    x = torch.zeros((42, 3), dtype=torch.float64, device="cuda")
    assert L.met2_bet_evolve(0, 8, 8, 8, dd.data_ptr(), vx, st, 0.4, 5, 1, x.data_ptr(), x.data_ptr(), None) == E_UNSUPPORTED
    assert L.met2_bet_evolve(0, 8, 8, 8, dd.data_ptr(), vx, st, 1.0, 1, 1, x.data_ptr(), x.data_ptr(), None) == E_INVALID
    assert L.met2_bet_evolve(0, 8, 8, 8, dd.data_ptr(), vx, st, 0.4, 1, 1, None, x.data_ptr(), None) == E_INVALID
    assert L.met2_bet_fill(0, 8, 8, 8, vx, -1, x.data_ptr(), 0, None, m.data_ptr(), None) == E_INVALID
    assert L.met2_bet_fill(0, 8, 8, 8, vx, 42, x.data_ptr(), 1, None, m.data_ptr(), None) == E_INVALID
    assert L.met2_bet_mean(0, 8, 0, dd.data_ptr(), dd.data_ptr(), None) == E_INVALID
    with pytest.raises(lib.Met2Error):
        motor.brain_mask_filter(np.ones((4, 4, 4)), (1.0, 1.0, 1.0))
    with pytest.raises(lib.Met2Error):
        motor.brain_mask_filter(dd, (1.0, 1.0, 1.0), level=5)


def driver_volume():
    """8 x 8 x 4 x 32: a two-pool decay in a bright block inside a dark rim, 1 % noise"""
    rng = np.random.default_rng(20261018)
    nx, ny, nz, nt = 8, 8, 4, 32
    TE = 10.0 * np.arange(1, nt + 1)
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    amp = np.where((np.abs(x - 3.6) < 2.8) & (np.abs(y - 3.4) < 2.8), 1000.0, 30.0)
    sig = amp[..., None] * (0.15 * np.exp(-TE / 20.0) + 0.85 * np.exp(-TE / 80.0))
    return sig * (1.0 + 0.01 * rng.standard_normal(sig.shape)), TE


def test_drivers_take_brain_mask(motor, bet, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    data, TE = driver_volume()
    vox = (8.0, 8.5, 10.0)                                               # the bright block is 48 x 51 x 40 mm
    args = (TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    mask = motor.brain_mask_filter(data, vox)
    assert 0 < mask.sum() < mask.size
    plain = motor.recon_met2_arrays(data, mask, *args)
    assert "mask" not in plain
    no = motor.recon_met2_arrays(data, mask, *args, brain_mask="no")
    assert sorted(no) == sorted(plain)
    for kw in ({}, {"devices": [0]}):
        got = motor.recon_met2_arrays(data, None, *args, brain_mask="yes", voxel_size=vox, **kw)
        assert sorted(got) == sorted(list(plain) + ["mask"])
        assert got["mask"].dtype == np.uint8 and np.array_equal(got["mask"], mask)
        for k in KEYS:
            assert np.array_equal(got[k], plain[k], equal_nan=True), (k, kw)
    # with degibbs='yes' the mean is taken of the unrung volume
    unrung = motor.gibbs_filter(data)
    mask_u = motor.brain_mask_filter(unrung, vox)
    both = motor.recon_met2_arrays(data, None, *args, brain_mask="yes", voxel_size=vox, degibbs="yes")
    want = motor.recon_met2_arrays(data, mask_u, *args, degibbs="yes")
    assert np.array_equal(both["mask"], mask_u)
    for k in KEYS:
        assert np.array_equal(both[k], want[k], equal_nan=True), k
    for kw, match in (({"brain_mask": "maybe"}, "brain_mask must be"), ({"brain_mask": "yes"}, "voxel_size"),
                      ({"brain_mask": "yes", "voxel_size": vox, "prepared": True}, "prepared"),
                      ({"brain_mask": "yes", "voxel_size": vox, "distributed": True}, "distributed")):
        with pytest.raises(ValueError, match=match):
            motor.recon_met2_arrays(data, None, *args, **kw)
    with pytest.raises(ValueError, match="does not go with a mask"):
        motor.recon_met2_arrays(data, mask, *args, brain_mask="yes", voxel_size=vox)
    # the on-disk driver takes the voxel size from the header and writes the mean and the mask
    aff = np.diag([8.0, -8.5, 10.0, 1.0])
    nifti.save(nifti.NiftiImage(data, aff), str(tmp_path / "data.nii.gz"))
    out = str(tmp_path) + "/bm_"
    res = motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), None, out, 3000.0, "X2", "L2", "None", "brute-force", "no", 40.0, 1,
                                 brain_mask="yes")
    for k in KEYS + ("mask", "Data_avg"):
        assert os.path.exists(out + k + ".nii.gz"), k
    assert np.array_equal(nifti.load(out + "mask.nii.gz").get_fdata(), mask) and np.array_equal(res["mask"], mask)
    assert np.array_equal(nifti.load(out + "Data_avg.nii.gz").get_fdata(), bet.bet_mean(data))
    assert np.array_equal(nifti.load(out + "MWF.nii.gz").get_fdata(), plain["MWF"])
    with pytest.raises(ValueError, match="path_to_mask"):
        motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), str(tmp_path / "data.nii.gz"), out, 3000.0, "X2", "L2", "None", "brute-force",
                               "no", 40.0, 1, brain_mask="yes")
    with pytest.raises(ValueError, match="brain_mask"):
        motor.motor_recon_met2(TE, str(tmp_path / "data.nii.gz"), None, out, 3000.0, "X2", "L2", "None", "brute-force", "no", 40.0, 1,
                               brain_mask="maybe")
