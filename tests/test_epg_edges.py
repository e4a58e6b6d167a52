"""The EPG dictionary (epg_dictionary_kernel) at the edges of what a plan accepts.

The fit tests at odd shapes read the dictionary back from the device and hand that same array to the CPU oracle, so a wrong
dictionary passes them.  Here the device's dictionary is compared with results that do not come from the device:
  CPU   the oracle's create_Dic_3D against tests/golden/golden_epg_edges.npz (the reference's own create_Dic_3D, epg/epg.py:155-162)
  2a    the device against that fixture
  2b    the device against the oracle (pinned by the CPU part) over a sweep of shapes, flip-angle counts, T1s and tau
  2c    the device against the closed form at alpha = 180 degrees, in np.longdouble
  2d    set_dictionary -> get_dictionary round trips (relayout_kernel in both directions)

Two measures: conftest.relmax over the whole array (the project's EPG bound, 1e-12) and col_err, the same per (T2, FA) column.  The
second is the stricter one: a column with T2 << tau is 1e-200 times smaller than the array's maximum and invisible to the first.
"""
import importlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN, relmax

PKG = "multicomponent-t2-toolbox_amd"
WHOLE_BOUND = 1e-12           # tests/test_gpu_parity.py::test_epg_dictionary_device
ORACLE_COL_BOUND = 1e-13      # oracle against the fixture, per column; measured 6.8e-15
# Device, per column: 10x the largest value measured on the MI355X against the fixture over all its cases, 7.08e-15 (32x60, alpha = 1e-3;
# the oracle shows 6.8e-15 at the same case).  The 10x covers the device's exp / sin / cos differing from the host's by an ulp or two,
# compounded over up to 126 half-periods.  Measured under this bound: 1.23e-14 against the oracle over the sweep (n_te = 63),
# 4.56e-15 against the closed form at alpha = 180.
DEVICE_COL_BOUND = 7.0e-14


def col_err(a, b):
    """[n_t2, n_fa]: max over the echoes of |a - b| / max over the echoes of |b|, per column of [n_te, n_t2, n_fa] dictionaries.
    A column that is all zero in b must be all zero in a (inf otherwise)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    den = np.max(np.abs(b), axis=0)
    num = np.max(np.abs(a - b), axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))


def edge_cases():
    g = np.load(os.path.join(GOLDEN, "golden_epg_edges.npz"))
    out = []
    for i in range(int(g["ncases"])):
        p = "c%d_" % i
        out.append({k: g[p + k] for k in ("T2s", "T1s", "alpha_values", "Dic")} | {"tau": float(g[p + "tau"]), "TR": float(g[p + "TR"])})
    return out


def edge_grids(n_t2):
    """The fixture's grids: T2 log-spaced from 0.5 ms (far below tau) to 2000 ms, a different T1 in every bin."""
    return np.logspace(np.log10(0.5), np.log10(2000.0), n_t2), np.linspace(300.0, 4000.0, n_t2)


def test_fixture_covers_the_edges():
    cs = edge_cases()
    ntes = {c["Dic"].shape[0] for c in cs}; nt2s = {c["Dic"].shape[1] for c in cs}
    angles = np.concatenate([c["alpha_values"] for c in cs])
    assert {2, 63} <= ntes and any(2 < n < 63 and n % 4 for n in ntes)
    assert nt2s & {2, 3} and nt2s & {64, 65} and 128 in nt2s
    assert all(np.ptp(c["T1s"]) > 0 and c["T2s"][0] * 5 < c["tau"] for c in cs)
    assert any(c["tau"] != 10.0 for c in cs) and any(c["TR"] != 3000.0 for c in cs)
    assert 0.0 in angles and 180.0 in angles and 179.999 in angles and (angles > 180.0).any() and ((angles > 0) & (angles < 90)).any()
    assert all(c["Dic"].shape == (c["Dic"].shape[0], c["T2s"].shape[0], c["alpha_values"].shape[0]) for c in cs)


def test_oracle_epg_against_reference_fixture(oracle):
    worst = 0.0
    for c in edge_cases():
        nte, nt2, nfa = c["Dic"].shape
        got = oracle.create_Dic_3D(nt2, c["T2s"], c["T1s"], nte, c["tau"], c["alpha_values"], c["TR"])
        e = col_err(got, c["Dic"])
        print("MEASURED epg_edges oracle-vs-fixture %dx%dx%d col=%.2e whole=%.2e" % (nte, nt2, nfa, e.max(), relmax(got, c["Dic"])))
        worst = max(worst, e.max())
        assert e.max() < ORACLE_COL_BOUND, (nte, nt2, e.max())             # measured 6.8e-15 (32x60, alpha = 1e-3)
        zero = c["alpha_values"] == 0.0
        assert not c["Dic"][:, :, zero].any() and not got[:, :, zero].any()
    print("MEASURED epg_edges oracle-vs-fixture worst col=%.2e" % worst)


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available()
    from oracle import oracle
    oracle.build()
    return importlib.import_module(PKG)


def device_dictionary(pkg, nte, T2s, T1s, tau, alphas, TR):
    alphas = np.atleast_1d(np.asarray(alphas, dtype=np.float64))
    plan = pkg.Met2Plan(nte, len(T2s), alphas.shape[0])
    try:
        return plan.build_dictionary_epg(T2s, T1s, tau, alphas, TR).get_dictionary()
    finally:
        plan.close()


@pytest.mark.gpu
def test_device_epg_against_reference_fixture(pkg):
    # 2a
    worst = 0.0
    for c in edge_cases():
        nte, nt2, nfa = c["Dic"].shape
        D = device_dictionary(pkg, nte, c["T2s"], c["T1s"], c["tau"], c["alpha_values"], c["TR"])
        e = col_err(D, c["Dic"]); w = relmax(D, c["Dic"])
        print("MEASURED epg_edges device-vs-fixture %dx%dx%d col=%.2e whole=%.2e" % (nte, nt2, nfa, e.max(), w))
        worst = max(worst, e.max())
        zero = c["alpha_values"] == 0.0
        assert not D[:, :, zero].any()                                     # alpha = 0: exact zeros, as the reference gives
        assert w < WHOLE_BOUND, (nte, nt2, w)
        assert e.max() < DEVICE_COL_BOUND, (nte, nt2, e.max())
    print("MEASURED epg_edges device-vs-fixture worst col=%.2e" % worst)


ODD_SHAPES = [(8, 12), (16, 20), (24, 40), (32, 64), (32, 65), (40, 96), (63, 128), (30, 33)]     # test_odd_shapes_vs_oracle's


def sweep_cases(nte):
    """(nte, T2s, T1s, tau, alphas, TR) of the sweep at one echo count: every n_t2 x n_fa x tau.  n_fa * n_t2 is the number of waves the
    kernel needs, four to a workgroup: 2 x 1, 63 x 1, 65 x 5, 127 x 273 ... leave a partial last workgroup, 64 x 1, 2 x 2, 128 x 273 fill it."""
    out = []
    for nt2 in (2, 63, 64, 65, 127, 128):
        T2s, T1s = edge_grids(nt2)
        for nfa in (1, 2, 5, 273):
            alphas = np.array([137.5]) if nfa == 1 else np.linspace(45.0, 200.0, nfa)
            for tau, TR in ((10.0, 3000.0), (6.7, 1200.0)):
                out.append((nte, T2s, T1s, tau, alphas, TR))
    return out


def _sweep(pkg, oracle, cases, tag):
    oracle.lib()                                                           # loaded before the threads ask for it
    worst_c = worst_w = 0.0
    with ThreadPoolExecutor(8) as pool:                                    # the oracle's C loop runs outside the interpreter lock
        refs = pool.map(lambda c: oracle.create_Dic_3D(len(c[1]), c[1], c[2], c[0], c[3], c[4], c[5]), cases)
        for c, ref in zip(cases, refs):
            D = device_dictionary(pkg, *c)
            e = col_err(D, ref).max(); w = relmax(D, ref)
            worst_c = max(worst_c, e); worst_w = max(worst_w, w)
            what = (c[0], len(c[1]), len(c[4]), c[3])
            assert D.shape == ref.shape and w < WHOLE_BOUND, (what, w)
            assert e < DEVICE_COL_BOUND, (what, e)
    print("MEASURED epg_edges device-vs-oracle %s cases=%d col=%.2e whole=%.2e" % (tag, len(cases), worst_c, worst_w))


@pytest.mark.gpu
@pytest.mark.parametrize("nte", [2, 3, 31, 32, 33, 62, 63])
def test_device_epg_against_oracle_sweep(pkg, nte):
    # 2b
    from oracle import oracle
    _sweep(pkg, oracle, sweep_cases(nte), "nte=%d" % nte)


@pytest.mark.gpu
def test_device_epg_at_the_odd_fit_shapes(pkg):
    # 2b: the dictionaries test_odd_shapes_vs_oracle reads back from the device and fits with on both sides, with its grid, T1, tau and angles
    from oracle import oracle
    synth = importlib.import_module(PKG + ".synth")
    cases = [(nte, synth.t2_grid(nt2), 1000.0 * np.ones(nt2), 10.0, np.linspace(120.0, 180.0, 7), 3000.0) for nte, nt2 in ODD_SHAPES]
    _sweep(pkg, oracle, cases, "odd-shapes")


@pytest.mark.gpu
def test_device_epg_closed_form_at_180(pkg):
    # 2c: perfect refocusing, D[e, j] = (1 - exp(-TR / T1_j)) exp(-(e + 1) tau / T2_j); no EPG code on the reference side at all
    nte, nt2, tau, TR = 63, 128, 10.0, 3000.0
    T2s, T1s = edge_grids(nt2)
    D = device_dictionary(pkg, nte, T2s, T1s, tau, [180.0], TR)[:, :, 0]
    ld = np.longdouble
    e = np.arange(1, nte + 1, dtype=ld)[:, None]
    ref = (1 - np.exp(-ld(TR) / T1s.astype(ld))) * np.exp(-e * ld(tau) / T2s.astype(ld))
    err = np.max(np.abs(D - ref), axis=0) / np.max(np.abs(ref), axis=0)
    print("MEASURED epg_edges device-vs-closed-form 63x128 alpha=180 col=%.2e" % float(err.max()))
    assert float(err.max()) < DEVICE_COL_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(63, 128, 273), (2, 2, 1), (30, 33, 7)])
def test_dictionary_layout_round_trip(pkg, shape):
    # 2d: [te][t2][fa] -> [fa][te][t2] -> [te][t2][fa]; every element distinct, so a wrong index shows
    rng = np.random.default_rng(sum(shape))
    Dic = rng.standard_normal(shape)
    assert np.unique(Dic).size == Dic.size
    plan = pkg.Met2Plan(*shape)
    back = plan.set_dictionary(Dic).get_dictionary()
    plan.close()
    assert np.array_equal(back, Dic)
