"""The three kernels of the Monte-Carlo study (csrc/met2_eval.hip) one by one, on inputs no fit produces and at every shape where they take
another path.  tests/test_gpu_evaluate.py runs them on fit outputs at two shapes; this module shows them the cases of tests/tools/eval_cases.py,
whose preconditions tests/test_eval_host.py asserts without a device.

met2_eval_voxel_metrics against tests/eval_ref.py (which test_eval_host.py holds to SciPy) at n_t2 = 3, 4, 5, 63, 64, 65, 127, 128: one and
two bins per lane, the sort padded to 4, 8, 64 and 128 or not at all, plateaus across bins 63 | 64.
  Equality.  On spectra of small integers with a power-of-two total every order of summation gives the same km, x, fM and fIE, so these and
  the peak count must EQUAL the restatement's; the peak count and the NaN / Inf pattern must be equal on every case, and the peak count equal
  to scipy.signal.find_peaks' wherever x holds numbers.  dist2 == x gives jsd == wd == mae == 0 exactly.
  Placement.  A voxel's nine values have the same bits in a launch of all cases, in the reversed launch, alone (n = 1), and in a launch without
  the NaN / Inf voxels.
  Rounding.  The file is compiled with contraction allowed, so the float fields are not asked for bit by bit: each is held to 16 x the largest
  relative error (against eval_ref run in long double) measured on an MI355X over these very cases (profiles/eval_parity.json, per quantity),
  and that bound may not exceed 1e-12.  test_eval_host.py asserts that float64 numpy is within 1e-13 of long double on every case, and SciPy's
  jensenshannon and wasserstein_distance on the seeded spectra; the device is compared with those two as well, at its bound + 1e-13.
met2_eval_reduce against eval_ref.reduce_metrics in long double at n = 1, 2, 255, 256, 257, 4099 (256 threads), with and without lam and fie,
the same rule with ceiling 1e-10; equal bits on a second call; and on degenerate columns (constant M or T, n = 1, T = 0 or 1, a NaN voxel)
the formulas' own NaN and Inf: R is NaN where pearsonr's is.
met2_synth_two_lobe against the header's recipe: the draws from an independent Philox4x32-10 (tests/tools/philox_numpy.py) within 2 ulp of
max(|lo|, |hi|) (one fused multiply-add against two roundings differs by less than 1 ulp: derived, not measured) for seeds and voxel ids that
fill every key and counter word; the Rician noise per (voxel, echo) from the device's own clean signal, in long double (16 x measured, ceiling
1e-12); the clean signal at n_te = 2, 32, 63 and n_t2 = 2, 64, 65, 128 against eval_ref.synth_clean and, at FA = 180, a closed form; grids
with bins beyond 300 ms and with a bin edge exactly on a point of the fine grid.
Every entry's refusals leave pre-filled outputs untouched.  With MET2_EVAL_PARITY_OUT=<file> the module writes what it measured there."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.spatial import distance
from scipy.stats import wasserstein_distance

import eval_ref
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import eval_cases as ec                                             # noqa: E402
import philox_numpy as ph                                           # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
LD = np.longdouble
INVALID, UNSUPPORTED, STATE = -1, -2, -5
FLOAT_FIELDS = {"fM": 0, "fIE": 1, "T2m": 2, "T2IE": 3, "km": 4, "mae_s": 6, "jsd": 7, "wd": 8}
CEILING = dict({k: 1e-12 for k in FLOAT_FIELDS}, reduce=1e-10, noise=1e-12)
MEASURED = {k: 0.0 for k in CEILING}
PROFILE = os.path.join(ROOT, "profiles", "eval_parity.json")
SCIPY_GATE = 1e-13                                                 # test_eval_host.test_conditioning_gate
FILL = -7.0


@pytest.fixture(scope="module")
def ev():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    ph.check_known_answers()
    yield importlib.import_module(PKG + ".evaluate")
    path = os.environ.get("MET2_EVAL_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"max_rel_error": MEASURED, "reference": "tests/eval_ref.py and the header's noise recipe in long double",
                       "measure": "max over the module's cases of |error| / |reference| per value (the noise: per voxel, over its first clean echo)",
                       "bound_factor": 16, "ceiling": CEILING, "device": torch.cuda.get_device_name(0)}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def L(ev):
    return importlib.import_module(PKG + "._lib").lib()


def bound(quantity):
    assert os.path.exists(PROFILE), "%s is missing: it holds the measured figures the bounds derive from" % PROFILE
    b = 16.0 * float(json.load(open(PROFILE))["max_rel_error"][quantity])
    assert b <= CEILING[quantity], "the measured error of %s puts the bound at %g: above %g it is a defect, not rounding" % (quantity, b, CEILING[quantity])
    return b


def held(quantity, err, what=""):
    """records the relative error `err` of `quantity`, prints it, and holds it to 16 x the figure measured on an MI355X"""
    MEASURED[quantity] = max(MEASURED[quantity], err) if np.isfinite(err) else MEASURED[quantity]
    print("%s %s: relative error %.3g" % (quantity, what, err))
    assert np.isfinite(err), (quantity, what, "a NaN, an Inf or an exact zero of the reference is not met")
    b = bound(quantity)
    assert err <= b, (quantity, what, err, b)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def grid_plan(n_te, T2s, cuts=None):
    """a plan that carries a T2 grid and the option cuts, nothing else"""
    plan = importlib.import_module(PKG).Met2Plan(n_te, T2s.shape[0], 1, device=0)
    plan.set_t2_grid(T2s)
    if cuts:
        plan.set_options(t2_myelin_cut=cuts[0], t2_ie_cut=cuts[1])
    return plan


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ================================================================ met2_eval_voxel_metrics

def metrics_ref(case, T2s, cuts, dtype=np.float64):
    """eval_ref.voxel_metrics in dtype; the peak count is a matter of exact float64 comparisons, so it is always the float64 restatement's"""
    with np.errstate(all="ignore"):
        m = eval_ref.voxel_metrics(case[2].astype(dtype), case[3].astype(dtype), T2s.astype(dtype), *cuts)
        if dtype != np.float64:
            m[5] = eval_ref.count_peaks(case[2] / np.sum(case[2]))
    return m


def launch(ev, plan, cases):
    out = ev.voxel_metrics(plan, dev(np.stack([c[2] for c in cases])), dev(np.stack([c[3] for c in cases])))
    torch.cuda.synchronize()
    return out.cpu().numpy()


_RUNS = {}


def metric_run(ev, n, which="default"):
    """cases, device output [9, ncase], float64 and long-double references of one bin count on one of three plans, computed once"""
    if (n, which) not in _RUNS:
        T2s = ec.t2_grid(n)
        grid, cuts = {"default": (T2s, (40.0, 200.0)), "other_cuts": (T2s, ec.other_cuts(T2s)), "above_ie": (ec.grid_above_ie(n), (40.0, 200.0))}[which]
        cases = ec.voxel_cases(n)
        plan = grid_plan(2, grid, None if cuts == (40.0, 200.0) else cuts)
        got = launch(ev, plan, cases)
        plan.close()
        r64 = np.stack([metrics_ref(c, grid, cuts) for c in cases], axis=1)
        rld = np.stack([metrics_ref(c, grid, cuts, LD) for c in cases], axis=1)
        r64.setflags(write=False); rld.setflags(write=False); got.setflags(write=False)
        _RUNS[(n, which)] = (cases, got, r64, rld, grid, cuts)
    return _RUNS[(n, which)]


@pytest.mark.parametrize("which", ["default", "other_cuts", "above_ie"])
@pytest.mark.parametrize("n", ec.N_T2)
def test_metrics_equalities(ev, n, which):
    cases, got, r64, _, grid, cuts = metric_run(ev, n, which)
    names = [c[0] for c in cases]
    np.testing.assert_array_equal(got[5], r64[5], err_msg="peaks %s" % names)
    for k in range(9):                                             # the NaN / Inf pattern of every field of every case
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(r64[k]), err_msg="NaN pattern of row %d %s" % (k, names))
        inf = np.isinf(r64[k])
        np.testing.assert_array_equal(got[k][inf], r64[k][inf])
        np.testing.assert_array_equal(np.isinf(got[k]), inf)
    ex = np.array([c[1] == "exact" for c in cases])
    assert ex.sum() >= 3
    for k in (0, 1, 4):
        np.testing.assert_array_equal(got[k][ex], r64[k][ex], err_msg="row %d on the exact-sum cases" % k)
    for v, c in enumerate(cases):
        with np.errstate(all="ignore"):
            x = c[2] / np.sum(c[2])
        if np.all(np.isfinite(x)):
            assert got[5, v] == signal.find_peaks(x, height=1e-5 * np.max(x))[0].size, c[0]
        if c[0].startswith("dist2_equals_x") or c[0] == "all_equal":
            assert got[6, v] == 0.0 and got[7, v] == 0.0 and got[8, v] == 0.0, (c[0], got[:, v])
    if which == "above_ie":                                        # no bin in either compartment: 0 / 1e-50
        fin = np.isfinite(r64[0])
        assert fin.sum() > len(cases) // 2 and np.all(got[:4, fin] == 0.0)
    if which == "default" and n >= 5:                              # the tie is a peak by hmin <= x; its twin, one level lower, is none
        tie = [got[5, names.index(k)] for k in names if k.startswith("tie@") or k == "tie"]
        twin = [got[5, names.index(k)] for k in names if k.startswith("tie_twin")]
        assert tie and len(tie) == len(twin) and all(a == b + 1 for a, b in zip(tie, twin))


@pytest.mark.parametrize("n", ec.N_T2)
def test_metrics_float_fields(ev, n):
    for which in ("default", "other_cuts", "above_ie"):
        cases, got, _, rld, _, _ = metric_run(ev, n, which)
        for q, k in FLOAT_FIELDS.items():
            held(q, ec.rel_err(got[k], rld[k]), "n_t2 %d %s" % (n, which))
    cases, got, _, _, _, _ = metric_run(ev, n)
    for v, c in enumerate(cases):
        if c[1] == "float":                                        # the well-conditioned cases against SciPy itself
            x = c[2] / np.sum(c[2])
            assert ec.rel_err(got[7, v], distance.jensenshannon(c[3], x)) <= bound("jsd") + SCIPY_GATE, c[0]
            assert ec.rel_err(got[8, v], wasserstein_distance(c[3], x)) <= bound("wd") + SCIPY_GATE, c[0]


@pytest.mark.parametrize("n", ec.N_T2)
def test_metrics_do_not_depend_on_the_launch(ev, n):
    cases, got, _, _, grid, _ = metric_run(ev, n)
    plan = grid_plan(2, grid)
    assert same_bits(launch(ev, plan, cases[::-1])[:, ::-1], got), "reversed launch"
    F, D = dev(np.stack([c[2] for c in cases])), dev(np.stack([c[3] for c in cases]))
    alone = torch.stack([ev.voxel_metrics(plan, F[v:v + 1], D[v:v + 1])[:, 0] for v in range(len(cases))], dim=1)
    torch.cuda.synchronize()
    assert same_bits(alone.cpu().numpy(), got), "n = 1"
    keep = [v for v, c in enumerate(cases) if not ec.has_nonfinite(c) and c[0] != "all_zero"]
    assert 0 < len(keep) < len(cases) - 5
    assert same_bits(launch(ev, plan, [cases[v] for v in keep]), got[:, keep]), "without the NaN / Inf / all-zero voxels"
    plan.close()


def test_metrics_refusals(ev, L):
    pkg = importlib.import_module(PKG)
    f, d, out = dev(np.ones((4, 8))), dev(np.full((4, 8), 0.125)), dev(np.full((9, 4), FILL))
    f2, d2 = dev(np.ones((4, 2))), dev(np.full((4, 2), 0.5))
    two = grid_plan(2, np.array([10.0, 100.0]))
    bare = pkg.Met2Plan(2, 8, 1, device=0)
    good = grid_plan(2, ec.t2_grid(8))
    assert L.met2_eval_voxel_metrics(two._h, 4, ptr(f2), ptr(d2), ptr(out), stream()) == UNSUPPORTED
    assert L.met2_eval_voxel_metrics(bare._h, 4, ptr(f), ptr(d), ptr(out), stream()) == STATE
    for a, b, c in ((None, d, out), (f, None, out), (f, d, None)):
        assert L.met2_eval_voxel_metrics(good._h, 4, ptr(a), ptr(b), ptr(c), stream()) == INVALID
    assert L.met2_eval_voxel_metrics(None, 4, ptr(f), ptr(d), ptr(out), stream()) == INVALID
    assert L.met2_eval_voxel_metrics(good._h, -1, ptr(f), ptr(d), ptr(out), stream()) == INVALID
    assert L.met2_eval_voxel_metrics(good._h, 0, ptr(None), ptr(None), ptr(None), stream()) == 0
    torch.cuda.synchronize()
    assert torch.all(out == FILL)
    assert L.met2_eval_voxel_metrics(good._h, 4, ptr(f), ptr(d), ptr(out), stream()) == 0
    torch.cuda.synchronize()
    assert torch.all(out[4] == 8.0)
    for p in (two, bare, good):
        p.close()


# ================================================================ met2_eval_reduce

def reduce_ld(pv, truth, lam, fie):
    with np.errstate(all="ignore"):
        return eval_ref.reduce_metrics(pv.astype(LD), truth.astype(LD), None if lam is None else lam.astype(LD), None if fie is None else fie.astype(LD))


def reduce_dev(ev, pv, truth, lam, fie):
    args = (dev(pv), dev(truth), None if lam is None else dev(lam), None if fie is None else dev(fie))
    a = ev.reduce_metrics(*args)
    b = ev.reduce_metrics(*args)
    assert same_bits(a, b), "a second call gives other bits"
    return a


@pytest.mark.parametrize("n", ec.REDUCE_N)
def test_reduce_matches_long_double(ev, n):
    pv, truth, lam, fie = ec.reduce_inputs(n)
    for use_lam in (True, False):
        for use_fie in (True, False):
            a = (pv, truth, lam if use_lam else None, fie if use_fie else None)
            got, want = reduce_dev(ev, *a), reduce_ld(*a)
            assert np.isnan(want[7]) == (n == 1)
            held("reduce", ec.rel_err(got, want), "n %d lam %s fie %s" % (n, use_lam, use_fie))
            if not use_lam:
                assert got[13] == 0.0 and got[14] == 0.0
    own = reduce_dev(ev, pv, truth, lam, None)
    assert same_bits(own, reduce_dev(ev, pv, truth, lam, pv[1].copy())), "fie = NULL reads the per-voxel fIE row"
    assert n == 1 or not same_bits(own, reduce_dev(ev, pv, truth, lam, fie))


def test_reduce_on_degenerate_columns(ev):
    """each aggregate is what its formula gives, NaN and Inf included (rel_err asks for the same NaN / Inf); R = 0/0 stays NaN"""
    plan = grid_plan(2, ec.t2_grid(8))
    nan_column = launch(ev, plan, [("z", "special", np.zeros(8), ec.default_dist2(8))])[:, 0]
    plan.close()
    assert np.isnan(nan_column[0]) and nan_column[4] == 0.0 and nan_column[5] == 0.0
    for name, a in ec.degenerate_reduce_inputs(nan_column).items():
        got, want = reduce_dev(ev, *a), reduce_ld(*a)
        if name.startswith("constant") or name == "n1" or name.startswith("nan_voxel"):
            assert np.isnan(want[7]) and np.isnan(got[7]), (name, got[7], "R of a constant or NaN column is NaN, not a clamped number")
        held("reduce", ec.rel_err(got, want), name)


def test_reduce_refusals(ev, L):
    pv, truth, out = dev(np.ones((9, 4))), dev(np.full((9, 4), 0.5)), dev(np.full((15,), FILL))
    assert L.met2_eval_reduce(0, ptr(pv), ptr(truth), ptr(None), ptr(None), ptr(out), stream()) == INVALID
    assert L.met2_eval_reduce(-3, ptr(pv), ptr(truth), ptr(None), ptr(None), ptr(out), stream()) == INVALID
    assert L.met2_eval_reduce(4, ptr(None), ptr(truth), ptr(None), ptr(None), ptr(out), stream()) == INVALID
    assert L.met2_eval_reduce(4, ptr(pv), ptr(None), ptr(None), ptr(None), ptr(out), stream()) == INVALID
    assert L.met2_eval_reduce(4, ptr(pv), ptr(truth), ptr(None), ptr(None), ptr(None), stream()) == INVALID
    torch.cuda.synchronize()
    assert torch.all(out == FILL)


# ================================================================ met2_synth_two_lobe

SEEDS = (0, 2 ** 31, 2 ** 32 + 5, 2 ** 63 + 1, -1)
# truth row -> (the draw's place among the eight uniforms of stream 1, its range's name)
DRAWS = {6: (0, "mwf"), 1: (1, "t2m"), 2: (2, "t2ie"), 4: (3, "fa"), 5: (4, "snr"), 7: (5, "sm"), 8: (6, "sie")}


def uniforms(seed, ids):
    """the eight 53-bit uniforms of stream 1 in the header's order, in long double [n, 8]: counter c0 = 0..3, two per counter"""
    x0, x1, x2, x3 = ph.voxel_words(seed, ids, np.arange(4), 1)
    u = np.empty((x0.shape[0], 8), dtype=LD)
    u[:, 0::2] = ph.u01_co(x0, x1, LD)
    u[:, 1::2] = ph.u01_co(x2, x3, LD)
    return u


def check_draws(ev, truth, seed, ids, snr, ranges, km=1000.0):
    r = dict(ev.RANGES, **ranges)
    u = uniforms(seed, ids)
    for row, (k, name) in DRAWS.items():
        if name == "snr":
            if snr is None:
                assert np.all(np.isinf(truth[5]) & (truth[5] > 0))
                continue
            lo, hi = snr
        else:
            lo, hi = r[name]
        want = LD(lo) + (LD(hi) - LD(lo)) * u[:, k]
        tol = 2.0 * np.spacing(max(abs(lo), abs(hi)))
        err = np.abs(truth[row].astype(LD) - want).max()
        assert err <= tol, (name, seed, float(err), tol)
        if lo == hi:
            assert np.all(truth[row] == lo)
        else:
            assert np.unique(truth[row]).size == truth.shape[1]
    assert np.all(truth[3] == km)


@pytest.mark.parametrize("seed", SEEDS)
def test_synth_draws_follow_the_header(ev, seed):
    plan = grid_plan(2, ec.t2_grid(8))
    n = 24
    for snr in ((50.0, 150.0), None):
        g = ev.synth_two_lobe(plan, n, seed=seed, snr=snr)
        torch.cuda.synchronize()
        check_draws(ev, g["truth"].cpu().numpy(), seed, np.arange(n), snr, {})
    narrow = dict(mwf=(0.125, 0.125), t2m=(20.0, 20.0 + 2.0 ** -20), t2ie=(70.0, 70.5), fa=(179.0, 180.0), sm=(2.0, 2.0), sie=(6.0, 6.0 + 2.0 ** -10))
    g = ev.synth_two_lobe(plan, n, seed=seed, snr=(20.0, 20.0), voxel_offset=1000, km=3.5, **narrow)
    torch.cuda.synchronize()
    check_draws(ev, g["truth"].cpu().numpy(), seed, 1000 + np.arange(n), (20.0, 20.0), narrow, km=3.5)
    plan.close()


def test_synth_voxel_ids_past_32_bits(ev):
    plan = grid_plan(8, ec.t2_grid(8))
    off, seed = 2 ** 32 - 3, 2 ** 63 + 1
    whole = ev.synth_two_lobe(plan, 8, seed=seed, voxel_offset=off)
    below = ev.synth_two_lobe(plan, 3, seed=seed, voxel_offset=off)
    above = ev.synth_two_lobe(plan, 5, seed=seed, voxel_offset=2 ** 32)
    low = ev.synth_two_lobe(plan, 5, seed=seed, voxel_offset=0)       # what a counter without the id's high word would give
    torch.cuda.synchronize()
    for k in ("data", "dist2"):
        assert torch.equal(whole[k], torch.cat([below[k], above[k]], dim=0)), k
    assert torch.equal(whole["truth"], torch.cat([below["truth"], above["truth"]], dim=1))
    assert not torch.equal(above["truth"], low["truth"]) and not torch.equal(above["data"], low["data"])
    check_draws(ev, whole["truth"].cpu().numpy(), seed, [off + v for v in range(8)], (50.0, 150.0), {})
    plan.close()


def noise_ld(clean, snr, seed, ids):
    """|S + sigma r cos t + i sigma r sin t| per (voxel, echo) in long double: sigma = S_0 / SNR, (r, t) from counter (e, 2, lo32(id), hi32(id)),
    the radius from the uniform in (0, 1], the angle from the one in [0, 1)"""
    nte = clean.shape[1]
    x0, x1, x2, x3 = ph.voxel_words(seed, ids, np.arange(nte), 2)
    r = np.sqrt(LD(-2.0) * np.log(ph.u01_oc(x0, x1, LD)))
    t = LD(6.283185307179586) * ph.u01_co(x2, x3, LD)
    S = clean.astype(LD)
    sg = (S[:, 0] / snr.astype(LD))[:, None]
    return np.sqrt((S + sg * r * np.cos(t)) ** 2 + (sg * r * np.sin(t)) ** 2)


@pytest.mark.parametrize("band", [(20.0, 20.0), (50.0, 150.0)])
@pytest.mark.parametrize("seed,off", [(3, 0), (-1, 2 ** 32 - 3)])
def test_synth_noise_follows_the_header(ev, band, seed, off):
    plan = grid_plan(32, ec.t2_grid(8))
    n = 48
    clean = ev.synth_two_lobe(plan, n, seed=seed, snr=None, voxel_offset=off)
    noisy = ev.synth_two_lobe(plan, n, seed=seed, snr=band, voxel_offset=off)
    torch.cuda.synchronize()
    S, X, tr = clean["data"].cpu().numpy(), noisy["data"].cpu().numpy(), noisy["truth"].cpu().numpy()
    assert not np.array_equal(S, X)
    want = noise_ld(S, tr[5], seed, [off + v for v in range(n)])
    err = float(np.max(np.abs(X.astype(LD) - want) / S[:, :1].astype(LD)))
    held("noise", err, "SNR %s seed %d offset %d" % (band, seed, off))
    plan.close()


def rel_rows(a, b):
    return np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)


@pytest.mark.parametrize("nt2", [2, 64, 65, 128])
@pytest.mark.parametrize("nte", [2, 32, 63])
def test_synth_clean_signal_at_the_shape_edges(ev, nte, nt2):
    T2s = ev.study_t2_grid(nt2)
    plan = grid_plan(nte, T2s)
    n = 3
    g = ev.synth_two_lobe(plan, n, seed=11, snr=None)
    flat = ev.synth_two_lobe(plan, n, seed=11, snr=None, fa=(180.0, 180.0))
    torch.cuda.synchronize()
    tr = g["truth"].cpu().numpy()
    data, d2, mwf = eval_ref.synth_clean(tr, nte, T2s)
    assert rel_rows(g["data"].cpu().numpy(), data).max() < 1e-12
    got_d2 = g["dist2"].cpu().numpy()
    assert rel_rows(got_d2, d2).max() < 1e-12
    # bins whose lower edge lies beyond 300 ms take no point of the fine grid: exact zeros (n_t2 = 2: the edge is 1005 ms)
    assert np.any(d2 == 0.0) and np.all(got_d2[d2 == 0.0] == 0.0) and np.all(got_d2[d2 > 0.0] > 0.0)
    np.testing.assert_allclose(tr[0], mwf, rtol=1e-12, atol=0)
    for v in range(n):                                             # the truth's MWF row is the sum of dist2 at T2 <= cut
        assert ec.rel_err(tr[0, v], np.sum(got_d2[v][T2s <= 40.0].astype(LD))) <= 1e-12
    # FA = 180: every echo e is km (1 - exp(-TR / T1)) sum_j pdf_j exp(-(e + 1) te / T2_j), independent of synth.epg_table
    ft = flat["truth"].cpu().numpy()
    assert np.all(ft[4] == 180.0) and same_bits(np.delete(ft, [0, 4], axis=0), np.delete(tr, [0, 4], axis=0))
    G = eval_ref.T2GRID.astype(LD)
    for v in range(n):
        z1, z2 = (G - LD(ft[1, v])) / LD(ft[7, v]), (G - LD(ft[2, v])) / LD(ft[8, v])
        pdf = LD(ft[6, v]) * np.exp(-z1 * z1 / 2) / LD(ft[7, v]) + (1 - LD(ft[6, v])) * np.exp(-z2 * z2 / 2) / LD(ft[8, v])
        pdf = pdf / pdf.sum()
        e = np.arange(1, nte + 1, dtype=LD)[:, None]
        want = LD(1000.0) * (1 - np.exp(LD(-3.0))) * np.sum(pdf[None, :] * np.exp(-e * LD(10.0) / G[None, :]), axis=1)
        got = flat["data"][v].cpu().numpy()
        assert float(np.max(np.abs(got - want)) / np.max(np.abs(want))) < 1e-12, (v, nte)
    plan.close()


def test_synth_bin_edge_on_a_fine_grid_point(ev):
    T2s, i, j = ec.midpoint_grid()
    assert T2s[i - 1] + (T2s[i] - T2s[i - 1]) / 2.0 == eval_ref.T2GRID[j]
    plan = grid_plan(2, T2s)
    centre = float(eval_ref.T2GRID[j])
    # a narrow intermediate lobe centred on the point: it carries a large share of the two bins, so the wrong side shows
    g = ev.synth_two_lobe(plan, 6, seed=4, snr=None, t2ie=(centre, centre), sie=(1.0, 1.0))
    torch.cuda.synchronize()
    tr, got = g["truth"].cpu().numpy(), g["dist2"].cpu().numpy()
    _, d2, mwf = eval_ref.synth_clean(tr, 2, T2s)
    assert rel_rows(got, d2).max() < 1e-12
    # moved to the lower bin, the point would change both bins by far more than that
    one = np.zeros(1000); one[j] = 1.0
    assert eval_ref.rebin(one, T2s)[i] == 1.0
    for v in range(6):
        dist = tr[6, v] * eval_ref._pdf(eval_ref.T2GRID, tr[1, v], tr[7, v]) + (1 - tr[6, v]) * eval_ref._pdf(eval_ref.T2GRID, tr[2, v], tr[8, v])
        share = dist[j] / dist.sum()
        assert share > 0.05 and abs(got[v, i] - d2[v, i]) < 1e-10 * share
    np.testing.assert_allclose(tr[0], mwf, rtol=1e-12, atol=0)
    plan.close()


def test_synth_refusals(ev, L):
    pkg = importlib.import_module(PKG)
    plan = grid_plan(4, ec.t2_grid(8))
    bare = pkg.Met2Plan(4, 8, 1, device=0)
    n = 3
    data, d2, truth = dev(np.full((n, 4), FILL)), dev(np.full((n, 8), FILL)), dev(np.full((9, n), FILL))
    Sp = importlib.import_module(PKG + "._lib").SynthParams

    def call(p, plan_=plan, n_=n, off=0, outs=(data, d2, truth)):
        return L.met2_synth_two_lobe(plan_._h if plan_ is not None else None, C.byref(p), n_, 5, off, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream())

    def params(**kw):
        p = ev.synth_params((50.0, 150.0))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert call(params(struct_size=C.sizeof(Sp) - 8)) == INVALID
    assert call(params(), n_=-1) == INVALID
    assert call(params(), off=-1) == INVALID
    assert call(params(t2m_hi=10.0)) == INVALID                    # hi < lo
    assert call(params(mwf_lo=float("nan"))) == INVALID
    assert call(params(sie_hi=float("inf"))) == INVALID
    assert call(params(snr_lo=0.0)) == INVALID
    assert call(params(snr_lo=100.0, snr_hi=50.0)) == INVALID
    assert call(params(te=0.0)) == INVALID
    assert call(params(t2m_lo=0.0)) == INVALID
    assert call(params(), outs=(None, d2, truth)) == INVALID
    assert call(params(), outs=(data, None, truth)) == INVALID
    assert call(params(), outs=(data, d2, None)) == INVALID
    assert call(params(), plan_=None) == INVALID
    assert call(params(), plan_=bare) == STATE
    assert call(params(), n_=0, outs=(None, None, None)) == 0
    torch.cuda.synchronize()
    assert torch.all(data == FILL) and torch.all(d2 == FILL) and torch.all(truth == FILL)
    assert call(params()) == 0
    torch.cuda.synchronize()
    assert torch.all(truth[3] == 1000.0) and torch.all(data > 0)
    plan.close(); bare.close()
