"""GPU: slice-profile-aware EPG dictionaries (epg_profile_dictionary_kernel, met2_plan_build_dictionary_epg_profile; include/met2_hip.h).
No expectation comes from the device: the comparison values are tests/tools/epg_profile_numpy.py, the loop of the entry's definition over
the CPU oracle's epg_signal (pinned in tests/test_epg_profile_host.py), and the CPU oracle's fits.
  degenerate   n_z = 1, r_exc = r_ref = w = [1.0]: the plain entry's dictionary, bit for bit (the shapes hold no -0 echo, the one value the
               definition's 0 + x would change: it would come back as +0)
  parity       per (T2, FA) column max_e |D - D_ref| <= 8e-14 S, S = scale sum_z w_z max_e |H_z[e]|: the project's DEVICE_COL_BOUND 7e-14
               (tests/test_epg_edges.py) on every term plus (n_z + 2) 2^-53 <= 7.4e-15 for the summation
  order        the same call twice and a profile padded with w = 0 points give the same bits
  invalid      MET2_E_INVALID, the plan's dictionary intact
  the point    on 2-D multi-slice data the plain dictionary loses the myelin peak and the flip angle, the profile dictionary finds both
  pipeline     recon_met2_arrays(slice_profile=p) is the run on a caller's plan built with p; None is a run without the argument
With MET2_EPG_PROFILE_PARITY_JSON set, the measured figures are kept in that file (profiles/epg_profile_parity.json was written this way)."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, relmax_rows

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import epg_profile_numpy as epn                                    # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
COL_BOUND = 8e-14
NZS = (1, 3, 4, 5, 33, 63, 64)
ANGLES = {1: [137.5], 2: [1e-3, 180.0], 3: [0.0, 150.0, 200.0], 7: [0.0, 1e-3, 45.0, 120.0, 179.999, 180.0, 200.0]}
_MEASURED = {}


def _keep(key, value):
    path = os.environ.get("MET2_EPG_PROFILE_PARITY_JSON")
    if not path:
        return
    _MEASURED[key] = value
    with open(path, "w") as f:
        json.dump(_MEASURED, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    from oracle import oracle
    oracle.build()
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def epg(pkg):
    return importlib.import_module(PKG + ".epg")


def grids(nt2):
    """tests/test_epg_edges.py's: T2 log-spaced from 0.5 ms (far below tau) to 2000 ms, a different T1 in every bin"""
    return np.logspace(np.log10(0.5), np.log10(2000.0), nt2), np.linspace(300.0, 4000.0, nt2)


def hann_profile(epg, n_z=31):
    rf = epg.hann_sinc(256, 2.7)
    return epg.pulse_pair_profile(rf, rf, 2.7, 2.7, n_z=n_z, z_max=1.5)


def random_profile(n_z, seed):
    """values in [0, 1.3], some r = 0 and some w = 0; the weights as drawn (not normalised: the entry uses them as given)"""
    rng = np.random.default_rng(seed)
    p = {"r_exc": rng.uniform(0.0, 1.3, n_z), "r_ref": rng.uniform(0.0, 1.3, n_z), "w": rng.uniform(0.0, 1.3, n_z)}
    if n_z >= 3:
        p["r_exc"][rng.integers(n_z)] = 0.0; p["r_ref"][rng.integers(n_z)] = 0.0
        p["w"][rng.integers(n_z - 1)] = 0.0
        p["w"][-1] = max(p["w"][-1], 0.1)
    p["r_ref"][0] = 1.3
    return p


def device_dictionary(pkg, nte, T2s, T1s, tau, alphas, TR, prof=None):
    plan = pkg.Met2Plan(nte, len(T2s), len(alphas))
    try:
        return plan.build_dictionary_epg(T2s, T1s, tau, alphas, TR, slice_profile=prof).get_dictionary()
    finally:
        plan.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ------------------------------------------------------------------------------------------ degenerate case
@pytest.mark.parametrize("shape", [(8, 5, 3), (32, 60, 7), (63, 128, 2)])
def test_one_point_profile_is_the_plain_dictionary(pkg, epg, shape):
    nte, nt2, nfa = shape
    T2s, T1s = grids(nt2)
    al = np.array(ANGLES[nfa])
    plain = device_dictionary(pkg, nte, T2s, T1s, 10.0, al, 1200.0)
    one = device_dictionary(pkg, nte, T2s, T1s, 10.0, al, 1200.0, {"r_exc": [1.0], "r_ref": [1.0], "w": [1.0]})
    assert plain.any() and np.isfinite(plain).all() and np.isfinite(one).all()
    nbits = int((bits(one) != bits(plain)).sum())
    print("MEASURED epg_profile degenerate %dx%dx%d: %d of %d entries differ in value, %d in bits" % (nte, nt2, nfa, int((one != plain).sum()), one.size, nbits))
    assert np.array_equal(bits(one), bits(plain))
    assert np.array_equal(bits(device_dictionary(pkg, nte, T2s, T1s, 10.0, al, 1200.0, epg.slice_profile([1.0], [1.0]))), bits(plain))


# ------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("shape", [(2, 2, 1), (31, 5, 3), (32, 60, 7), (48, 120, 3), (63, 128, 2)])
def test_parity_with_the_definition(pkg, epg, shape):
    nte, nt2, nfa = shape
    T2s, T1s = grids(nt2)
    al = np.array(ANGLES[nfa])
    tau, TR = (10.0, 1000.0) if nte != 31 else (6.7, 1200.0)
    worst, alive = 0.0, 0
    for n_z in NZS:
        for kind, prof in (("hann", hann_profile(epg, n_z)), ("random", random_profile(n_z, 1000 * nte + n_z))):
            D = np.transpose(device_dictionary(pkg, nte, T2s, T1s, tau, al, TR, prof), (2, 0, 1))
            ref, S = epn.dictionary_fa_major(nt2, T2s, T1s, nte, tau, al, TR, prof["r_exc"], prof["r_ref"], prof["w"], want_scale=True)
            err = np.max(np.abs(D - ref), axis=1)                       # [fa][t2]
            assert np.isfinite(D).all()
            alive += bool(ref.any())                                    # (a random profile whose only weighted point has r_ref = 0 gives all zeros)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(S > 0, err / S, np.where(err > 0, np.inf, 0.0))
            worst = max(worst, float(rel.max()))
            assert np.all(err <= COL_BOUND * S), (shape, n_z, kind, float(rel.max()))
            zero = al == 0.0
            assert not D[zero].any()                                    # alpha = 0: exact zeros
    assert alive >= 2 * len(NZS) - 2
    print("MEASURED epg_profile parity %dx%dx%d worst max_e|D - D_ref| / S = %.2e (bound %.1e)" % (nte, nt2, nfa, worst, COL_BOUND))
    _keep("parity/%dx%dx%d" % shape, {"worst_err_over_S": worst, "bound": COL_BOUND, "n_z": list(NZS)})


# ------------------------------------------------------------------------------------------ order and launch independence
@pytest.mark.parametrize("shape", [(32, 60, 7), (63, 128, 2)])
def test_same_bits_twice_and_under_zero_weight_padding(pkg, shape):
    nte, nt2, nfa = shape
    T2s, T1s = grids(nt2)
    al = np.array(ANGLES[nfa])
    for n_z in (3, 5, 33):
        prof = random_profile(n_z, 7 + n_z)
        a = device_dictionary(pkg, nte, T2s, T1s, 10.0, al, 1000.0, prof)
        b = device_dictionary(pkg, nte, T2s, T1s, 10.0, al, 1000.0, prof)
        assert np.array_equal(bits(a), bits(b))
        for pad in (1, 2, 64 - n_z):                                     # other waves take other points; the sum keeps its order
            rng = np.random.default_rng(pad)
            padded = {"r_exc": np.concatenate([prof["r_exc"], rng.uniform(0, 1.3, pad)]), "r_ref": np.concatenate([prof["r_ref"], rng.uniform(0, 1.3, pad)]),
                      "w": np.concatenate([prof["w"], np.zeros(pad)])}
            c = device_dictionary(pkg, nte, T2s, T1s, 10.0, al, 1000.0, padded)
            assert np.array_equal(bits(a), bits(c)), (shape, n_z, pad)


# ------------------------------------------------------------------------------------------ invalid arguments
def test_invalid_arguments_leave_the_plan_alone(pkg, epg):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    nte, nt2 = 8, 5
    T2s, T1s = grids(nt2)
    al = np.array([120.0, 180.0])
    plan = pkg.Met2Plan(nte, nt2, 2)
    good = random_profile(4, 3)
    before = plan.build_dictionary_epg(T2s, T1s, 10.0, al, 1000.0, slice_profile=good).get_dictionary()
    dp = C.POINTER(C.c_double)
    h = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    fixed = [h(T2s), h(T1s), h(al)]

    def call(n_z, r_exc, r_ref, w):
        arrs = [None if a is None else h(a) for a in (r_exc, r_ref, w)]
        ptr = [None if a is None else a.ctypes.data_as(dp) for a in arrs]
        return L.met2_plan_build_dictionary_epg_profile(plan._h, fixed[0].ctypes.data_as(dp), fixed[1].ctypes.data_as(dp), 10.0, fixed[2].ctypes.data_as(dp),
                                                        1000.0, n_z, ptr[0], ptr[1], ptr[2], None)

    ones = np.ones(65)
    bad = [(0, ones, ones, ones), (65, ones, ones, ones), (-1, ones, ones, ones), (2, [1.0, np.nan], [1.0, 1.0], [0.5, 0.5]), (2, [1.0, 1.0], [np.inf, 1.0], [0.5, 0.5]),
           (2, [1.0, 1.0], [1.0, 1.0], [np.nan, 0.5]), (2, [1.0, -0.5], [1.0, 1.0], [0.5, 0.5]), (2, [1.0, 1.0], [1.0, -1e-300], [0.5, 0.5]),
           (2, [1.0, 1.0], [1.0, 1.0], [1.0, -1.0]), (3, [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]), (2, None, ones, ones), (2, ones, None, ones),
           (2, ones, ones, None)]
    for args in bad:
        assert call(*args) == -1, args                                  # MET2_E_INVALID
        assert L.met2_last_error()
        assert np.array_equal(bits(plan.get_dictionary()), bits(before)), args
    with pytest.raises(pkg.Met2Error):
        plan.build_dictionary_epg(T2s, T1s, 10.0, al, 1000.0, slice_profile={"r_exc": [1.0, 1.0], "r_ref": [1.0, 1.0], "w": [0.0, 0.0]})
    with pytest.raises(ValueError):
        plan.build_dictionary_epg(T2s, T1s, 10.0, al, 1000.0, slice_profile={"r_exc": [1.0, 1.0], "r_ref": [1.0], "w": [0.5, 0.5]})
    assert np.array_equal(bits(plan.get_dictionary()), bits(before)) and epg.same_profile(plan.slice_profile, good)
    assert call(4, good["r_exc"], good["r_ref"], good["w"]) == 0         # and a valid call still goes through
    assert np.array_equal(bits(plan.get_dictionary()), bits(before))
    plan.close()


# ------------------------------------------------------------------------------------------ the feature's point
NTE, NT2, TAU, TR = 32, 60, 10.0, 1000.0
CENTRE = np.array([120.0, 140.0, 160.0, 180.0])
ALPHAS = np.linspace(90.0, 180.0, 91)


def two_pool_through_profile(prof, centre, per_angle, seed):
    """noiseless voxels of a 20 / 80 ms two-pool tissue (MWF 0.15) seen through the slice profile at the centre angles, amplitudes 100..1000:
    [len(centre) * per_angle, NTE] and the index of every voxel's centre angle on the 90..180 grid"""
    G = epn.dictionary_fa_major(2, [20.0, 80.0], [1000.0, 1000.0], NTE, TAU, centre, TR, prof["r_exc"], prof["r_ref"], prof["w"])
    sig = 0.15 * G[:, :, 0] + 0.85 * G[:, :, 1]
    amp = np.random.default_rng(seed).uniform(100.0, 1000.0, (len(centre), per_angle))
    data = (sig[:, None, :] * amp[:, :, None]).reshape(-1, NTE)
    return np.ascontiguousarray(data), np.repeat(np.round(centre - 90.0).astype(int), per_angle)


def test_profile_dictionary_recovers_flip_angle_and_myelin(pkg, epg):
    """CPU oracle on the same data: the plain 91-angle dictionary gives FA 90 / 100 / 111 / 121 degrees for the centre angles 120 / 140 / 160 / 180
    and MWF 0.000; the profile dictionary the true angle and MWF 0.117 .. 0.126."""
    import torch
    from oracle import oracle
    synth = importlib.import_module(PKG + ".synth")
    prof = hann_profile(epg)
    data_h, true_idx = two_pool_through_profile(prof, CENTRE, 64, 5)
    data = torch.as_tensor(data_h, device="cuda")
    T2s = synth.t2_grid(NT2); T1s = 1000.0 * np.ones(NT2)
    L = oracle.penalty(NT2, "L2")
    ones = np.ones(len(data_h))
    got = {}
    for name, p in (("profile", prof), ("plain", None)):
        plan = pkg.Met2Plan(NTE, NT2, 91)
        plan.build_dictionary_epg(T2s, T1s, TAU, ALPHAS, TR, slice_profile=p).set_penalty("L2", T2s)
        fa, _, _ = plan.fa_bruteforce(data)
        out = plan.fit("X2", data, fa_index=fa)
        D = np.ascontiguousarray(np.transpose(plan.get_dictionary(), (2, 0, 1)))
        plan.close()
        fa = fa.cpu().numpy().astype(int)
        mwf = out["maps"][0].cpu().numpy()
        fs, _, _, _ = oracle.fit_batch("X2", D, L, data_h, fa.astype(np.float64), ones, nthreads=8)
        e = relmax_rows(out["fsol"].cpu().numpy(), fs)
        mwf_o = oracle.metrics(fs, T2s, ones)["MWF"]
        print("MEASURED epg_profile point %s: FA %s  MWF %.4f .. %.4f  fsol vs oracle %.2e  MWF vs oracle %.2e"
              % (name, sorted(set(ALPHAS[fa].tolist())), mwf.min(), mwf.max(), e.max(), np.abs(mwf - mwf_o).max()))
        _keep("point/" + name, {"FA_deg": sorted(set(ALPHAS[fa].tolist())), "MWF_min": float(mwf.min()), "MWF_max": float(mwf.max()),
                                "fsol_vs_oracle": float(e.max())})
        got[name] = (fa, mwf, e, np.abs(mwf - mwf_o))
    fa, mwf, e, dm = got["profile"]
    assert np.array_equal(fa, true_idx)
    assert np.all(mwf > 0.10)
    assert e.max() < 1e-5 and dm.max() < 1e-5
    fa, mwf, e, dm = got["plain"]
    assert np.all(np.abs(ALPHAS[fa] - ALPHAS[true_idx]) >= 20.0)
    assert np.all(mwf < 0.01)
    assert e.max() < 1e-5 and dm.max() < 1e-5


# ------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def volume(epg):
    prof = hann_profile(epg)
    data, idx = two_pool_through_profile(prof, np.array([130.0, 150.0]), 128, 9)
    data = data.reshape(8, 8, 4, NTE)
    mask = np.ones((8, 8, 4)); mask[0, 0, :] = 0; mask[3, 5, 2] = 0
    return prof, data, mask, idx.reshape(8, 8, 4) + 90.0


@pytest.mark.parametrize("FA_method", ["spline", "brute-force"])
def test_pipeline_routes_the_profile(pkg, volume, FA_method):
    motor = importlib.import_module(PKG + ".motor")
    prof, data, mask, centre = volume
    te = TAU * np.arange(1, NTE + 1)
    kw = dict(FA_method=FA_method)
    if FA_method == "brute-force":
        kw["bootstrap"] = dict(n_rep=4, seed=1)                         # fa='fixed': the replicates are refitted on the run's own dictionary
    own = motor.recon_met2_arrays(data, mask, te, TR, slice_profile=prof, **kw)
    n_fa = 273 if FA_method == "spline" else 91
    plan = pkg.Met2Plan(NTE, 60, n_fa, myelin_T2=40.0)
    T2s = np.logspace(np.log10(10.0), np.log10(2000.0), 60)
    plan.build_dictionary_epg(T2s, 1000.0 * np.ones(60), TAU, np.linspace(90.0, 180.0, n_fa), TR, slice_profile=prof).set_penalty("L2", T2s)
    theirs = motor.recon_met2_arrays(data, mask, te, TR, plan=plan, **kw)
    again = motor.recon_met2_arrays(data, mask, te, TR, plan=plan, slice_profile=prof, **kw)
    with pytest.raises(ValueError, match="slice_profile differs"):
        motor.recon_met2_arrays(data, mask, te, TR, plan=plan, slice_profile=dict(prof, r_ref=0.5 * prof["r_ref"]), **kw)
    plan.close()
    assert set(own) == set(theirs) == set(again)
    for k in own:
        assert np.array_equal(own[k], theirs[k], equal_nan=True), k
        assert np.array_equal(own[k], again[k], equal_nan=True), k
    m = mask > 0
    # brute force: the grid holds the centre angles, so the index is exact (as on the voxel list above); spline: the minimum of a cubic through
    # the 15 coarse residuals, good to a fraction of the coarse spacing -- half of it is asked (the CPU oracle is off by 0.2 .. 1.0 degrees)
    fa_bound = 0.0 if FA_method == "brute-force" else 0.5 * 90.0 / 14.0
    print("MEASURED epg_profile pipeline %s: max |FA - centre| = %.3f deg, MWF %.4f .. %.4f" % (FA_method, np.abs(own["FA"] - centre)[m].max(),
                                                                                               own["MWF"][m].min(), own["MWF"][m].max()))
    assert np.abs(own["FA"] - centre)[m].max() <= fa_bound + 1e-9
    assert np.all(own["MWF"][m] > 0.10) and not own["MWF"][~m].any()
    plain = motor.recon_met2_arrays(data, mask, te, TR, FA_method=FA_method)
    none = motor.recon_met2_arrays(data, mask, te, TR, FA_method=FA_method, slice_profile=None)
    assert set(plain) == set(none)
    for k in plain:
        assert np.array_equal(plain[k], none[k], equal_nan=True), k
    assert np.all(np.abs(plain["FA"] - centre)[m] >= 20.0) and np.all(plain["MWF"][m] < 0.01)
