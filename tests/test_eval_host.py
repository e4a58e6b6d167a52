"""CPU tests of the Monte-Carlo study (met2_amd.evaluate): the numpy restatement tests/eval_ref.py against SciPy on adversarial spectra
(the GPU kernels are checked against eval_ref in test_gpu_evaluate.py and test_gpu_eval_kernels.py), the table writer against the reference's
committed tables, and the preconditions of the cases test_gpu_eval_kernels.py shows the kernels (tests/tools/eval_cases.py): exact sums, the
threshold tie and its twin, the NaN patterns, the conditioning gate, the reduction's degenerate columns, the bin edge on a fine grid point."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

import eval_ref
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import eval_cases as ec                                             # noqa: E402
import philox_numpy as ph                                           # noqa: E402
from eval_cases import adversarial_spectra                          # noqa: E402  (moved there; the GPU tests of the kernels share them)

PKG = "multicomponent-t2-toolbox_amd"


def fixture():
    with open(os.path.join(GOLDEN, "eval_tables_paper.json")) as f:
        return json.load(f)


def test_peaks_match_scipy():
    signal = pytest.importorskip("scipy.signal")
    for x in adversarial_spectra():
        peaks, _ = signal.find_peaks(x, height=1e-5 * np.max(x))
        assert eval_ref.count_peaks(x) == peaks.size, x


def test_jsd_and_wasserstein_match_scipy():
    pytest.importorskip("scipy")
    from scipy.spatial import distance
    from scipy.stats import wasserstein_distance
    rng = np.random.default_rng(11)
    xs = adversarial_spectra()
    for x in xs:
        for p in (rng.random(x.shape[0]), np.where(rng.random(x.shape[0]) < 0.3, 0.0, rng.random(x.shape[0])), x[::-1].copy(), x.copy()):
            js = distance.jensenshannon(p, x)
            assert abs(eval_ref.jensenshannon(p, x) - js) <= 1e-12 * max(1.0, js), (p, x)
            wd = wasserstein_distance(p, x)
            assert abs(eval_ref.wasserstein(p, x) - wd) <= 1e-12 * max(wd, 1e-300) + 1e-17, (p, x)


def test_rebin_matches_the_reference_loop():
    T2grid, dT2grid = np.linspace(1.0, 300.0, 1000, retstep=True)
    for npc in (60, 120):
        T2s = np.logspace(np.log10(10.0), np.log10(2000.0), npc)
        rng = np.random.default_rng(npc)
        dist = rng.random(1000)
        dist /= dist.sum()
        # :404-426, literally
        dist2 = np.zeros(npc)
        T2_delta_max = T2s[0] + (T2s[1] - T2s[0]) / 2.0
        dist2[0] = np.sum(dist[T2grid < T2_delta_max] * dT2grid)
        for it in range(1, npc - 1):
            lo = T2s[it - 1] + (T2s[it] - T2s[it - 1]) / 2.0
            hi = T2s[it] + (T2s[it + 1] - T2s[it]) / 2.0
            dist2[it] = np.sum(dist[(T2grid >= lo) & (T2grid < hi)] * dT2grid)
        dist2[npc - 1] = np.sum(dist[T2grid >= T2s[npc - 2] + (T2s[npc - 1] - T2s[npc - 2]) / 2.0] * dT2grid)
        dist2 = dist2 / np.sum(dist2)
        np.testing.assert_array_equal(eval_ref.rebin(dist, T2s), dist2)


def test_aggregates_match_the_reference_formulas():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(3)
    n = 5000
    T = rng.uniform(0.05, 0.25, n)
    truth = np.stack([T, rng.uniform(15, 35, n), rng.uniform(60, 90, n), np.full(n, 1000.0)])
    pv = np.stack([T + rng.normal(0, 0.03, n), 1 - T + rng.normal(0, 0.03, n), truth[1] * rng.uniform(0.8, 1.2, n), truth[2] * rng.uniform(0.9, 1.1, n),
                   1000 * rng.uniform(0.95, 1.05, n), rng.integers(1, 5, n).astype(float), rng.random(n) * 0.02, rng.random(n), rng.random(n) * 0.01])
    lam = rng.lognormal(-3, 2, n)
    fie_nnls = 1 - T + rng.normal(0, 0.05, n)
    got = eval_ref.reduce_metrics(pv, truth, lam, fie_nnls)
    # compute_multi_metrics (:77-123) as the reference writes it, with its NNLS fIE array in GMARE's second term
    MWF, Mie = pv[0], fie_nnls
    residual = MWF - T
    RMSE = np.sqrt(np.mean(residual ** 2))
    R, _ = stats.pearsonr(MWF.flatten(), T.flatten())
    want = [np.mean(np.abs(residual)), np.mean(np.abs(residual / T)), RMSE,
            np.sqrt(np.mean(((MWF - np.mean(MWF)) - (T - np.mean(T))) ** 2)), np.sqrt(np.mean((residual / T) ** 2)),
            1.96 * np.sqrt(np.std(residual) ** 2 + RMSE ** 2), np.mean(residual), R,
            np.mean(np.abs(residual / T)) + np.mean(np.abs(Mie - (1.0 - T)) / (1.0 - T)) + np.mean(np.abs(pv[2] - truth[1]) / truth[1])
            + np.mean(np.abs(pv[3] - truth[2]) / truth[2]) + np.mean(np.abs(pv[4] - truth[3]) / truth[3]),
            np.mean(np.abs(pv[5] - 2.0)), np.mean(pv[6]), np.mean(pv[7]), np.mean(pv[8]), np.mean(lam), np.std(lam)]
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)


def test_voxel_metrics_on_degenerate_spectra():
    T2s = np.logspace(1, np.log10(2000.0), 60)
    d2 = np.exp(-0.5 * ((np.log(T2s) - np.log(70)) / 0.2) ** 2)
    d2 /= d2.sum()
    f = np.zeros(60)
    f[20] = 500.0                                                              # one non-zero bin: one peak, all of it in one compartment
    m = eval_ref.voxel_metrics(f, d2, T2s)
    assert m[4] == 500.0 and m[5] == 1
    assert (m[0] == 1.0) == (T2s[20] <= 40.0) and (m[1] == 1.0) == (40.0 < T2s[20] <= 200.0)
    m0 = eval_ref.voxel_metrics(np.zeros(60), d2, T2s)                         # an all-zero fit: nan metrics (0/0) and no peaks
    assert np.isnan(m0[0]) and m0[5] == 0 and np.isnan(m0[7])


def test_fixture_holds_three_bands_of_ten_methods():
    ev = importlib.import_module(PKG + ".evaluate")
    fx = fixture()
    assert tuple(fx["error_columns"]) == ev.ERROR_COLUMNS and tuple(fx["regularization_columns"]) == ev.REG_COLUMNS
    assert sorted(fx["bands"]) == ["150_300", "50_150", "inf"]
    for b in fx["bands"].values():
        assert tuple(b["methods"]) == ev.PAPER_METHODS
        assert np.asarray(b["errors"]).shape == (10, 13) and np.asarray(b["regularization"]).shape == (10, 2)


def test_write_tables_reproduces_the_reference_layout(tmp_path):
    ev = importlib.import_module(PKG + ".evaluate")
    for key, b in fixture()["bands"].items():
        sha = lambda p: hashlib.sha256(p.read_bytes()).hexdigest()
        # the .txt tables from the numbers they print (6 significant digits), the .csv from theirs (4 decimals; full-precision lambdas)
        a, c = tmp_path / (key + "_txt"), tmp_path / (key + "_csv")
        ev.EvalResult(b["methods"], b["errors"], b["regularization"]).write_tables(str(a))
        ev.EvalResult(b["methods"], b["errors_csv"], b["regularization_csv"]).write_tables(str(c))
        assert sha(a / "table_errors.txt") == b["sha256"]["table_errors.txt"], key
        assert sha(a / "table_regularization.txt") == b["sha256"]["table_regularization.txt"], key
        assert sha(c / "table_errors.csv") == b["sha256"]["table_errors.csv"], key
        assert sha(c / "table_regularization.csv") == b["sha256"]["table_regularization.csv"], key


def test_format_table_aligns_like_tabulate():
    ev = importlib.import_module(PKG + ".evaluate")
    text = ev.format_table(("Method", "a", "bb"), [["x", 1.5, -2e-7], ["long label", 0, 123.25]])
    assert text.splitlines() == ["Method        a       bb",
                                 "----------  ---  -------",
                                 "x           1.5   -2e-07",
                                 "long label  0    123.25"]


def test_study_grids_and_params():
    ev = importlib.import_module(PKG + ".evaluate")
    lam = ev.study_lambda_grid()
    assert lam.shape == (50,) and lam[0] == 0.0 and lam[1] == 1e-8 and abs(lam[-1] - 100.0) < 1e-12
    p = ev.synth_params(None)
    assert p.snr_lo == np.inf and p.fa_lo == 90.0 and p.fa_hi == 180.0 and p.km == 1000.0
    with pytest.raises(ValueError):
        ev.synth_params((50, 150), bogus=(1, 2))
    with pytest.raises(ValueError):
        ev.evaluate_methods(methods=("11. nonsense",))


# ---------------------------------------------------------------- the preconditions of tests/test_gpu_eval_kernels.py, checked without a device

LD = np.longdouble
GATE = 1e-13


def metrics_ref(case, T2s, cuts=(40.0, 200.0), dtype=np.float64):
    """eval_ref.voxel_metrics in dtype.  The peak count is a matter of exact float64 comparisons (a tie at the height threshold is no tie in
    long double), so it is always the float64 restatement's."""
    with np.errstate(all="ignore"):
        m = eval_ref.voxel_metrics(case[2].astype(dtype), case[3].astype(dtype), T2s.astype(dtype), *cuts)
        if dtype != np.float64:
            m[5] = eval_ref.count_peaks(case[2] / np.sum(case[2]))
    return m


def test_philox_restatement_and_uniform_rules():
    ph.check_known_answers()
    top = 0xFFFFFFFF
    assert ph.u01_co(0, 0) == 0.0 and ph.u01_co(top, top) == 1.0 - 2.0 ** -53
    assert ph.u01_oc(0, 0) == 2.0 ** -53 and ph.u01_oc(top, top) == 1.0
    assert ph.u01_co(1 << 5, 0) == 2.0 ** -27 and ph.u01_co(0, 1 << 6) == 2.0 ** -53 and ph.u01_co(31, 63) == 0.0
    assert ph.u01_co(top, 12345, LD) == ph.u01_co(top, 12345) and ph.u01_oc(top, 12345, LD) == ph.u01_oc(top, 12345)
    lo, hi = ph.halves([0, 2 ** 31, 2 ** 32 + 5, 2 ** 63 + 1, -1, 2 ** 32 - 3])
    assert lo.tolist() == [0, 2 ** 31, 5, 1, top, top - 2] and hi.tolist() == [0, 0, 1, 2 ** 31, top, 0]
    # voxel_words is philox4x32_10 at counter (c0, stream, lo32(id), hi32(id)) under key (lo32(seed), hi32(seed))
    w = ph.voxel_words(-1, [2 ** 32 + 7], [3], 2)
    assert ph.words(*(x[0, 0] for x in w)) == ph.words(*ph.philox4x32_10([3, 2, 7, 1], [top, top]))


def test_exact_sum_cases_are_exact_and_have_their_structure():
    signal = pytest.importorskip("scipy.signal")
    for n in ec.N_T2:
        T2s = ec.t2_grid(n)
        names = {}
        for name, f in ec.exact_spectra(n):
            for cuts in ((40.0, 200.0), ec.other_cuts(T2s)):
                km, x = ec.assert_exact_sums(f, T2s, *cuts)
                m = eval_ref.voxel_metrics(f, ec.default_dist2(n), T2s, *cuts)
                assert m[4] == km and m[0] == np.sum(x[T2s <= cuts[0]]) and m[1] == np.sum(x[(T2s > cuts[0]) & (T2s <= cuts[1])])
            peaks, _ = signal.find_peaks(x, height=1e-5 * np.max(x))
            assert eval_ref.count_peaks(x) == peaks.size, (n, name)
            names[name] = peaks.size
        assert len(names) >= (3 if n == 3 else 20), (n, len(names))
        if n >= 10:
            want = {"plateau_from_1": 1, "plateau_from_1_long": 1, "plateau_into_last": 0, "plateau_into_last_long": 0, "peak_at_n-2": 1,
                    "peak_at_n-2_and_1": 2, "endpoints_only": 0, "plateaus@0": 2, "single@0": 1, "endpoints@0": 1,
                    "plateau_to_end@%d" % (n - 10): 0, "plateau_to_end@0": 1, "threshold_ties@0": 4, "zigzag@%d" % (n - 10): 3}
            if n >= 65:
                want["plateau_61..64"] = 0 if n == 65 else 1
            if n >= 66:
                want.update({"plateau_62..65": 1, "plateau_63..64": 1, "step_up_63_64": 1, "plateau_1..64": 1})
            if n >= 68:
                assert any(k.endswith("@58") for k in names)        # 58..67 straddles 62..66
            for k, v in want.items():
                assert names[k] == v, (n, k, names[k], v)
        else:
            assert set(np.unique(list(names.values()))) >= ({0, 1} if n < 5 else {0, 1, 2})


def test_threshold_tie_and_its_twin():
    signal = pytest.importorskip("scipy.signal")
    assert 1e-5 * (ec.BIG / ec.TOTAL) == 1.0 / ec.TOTAL and 1e-5 * (2 * ec.BIG / (2 * ec.TOTAL)) == 2.0 / (2 * ec.TOTAL)
    for tie, two, twin, npk in ((ec.TIE10, ec.TIE10_TWO, ec.TIE10_TWIN, 3), (ec.TIE5, ec.TIE5_TWO, ec.TIE5_TWIN, 2)):
        for f, want in ((tie, npk), (two, npk), (twin, npk - 1)):
            f = np.asarray(f, dtype=np.float64)
            assert ec.is_pow2(float(f.sum()))
            x = f / f.sum()
            b = len(f) - 4 if len(f) == 10 else 3                  # the bin on (or one level under) the threshold
            hmin = 1e-5 * np.max(x)
            assert (x[b] == hmin) == (want == npk) and (want == npk or x[b] < hmin)
            assert eval_ref.count_peaks(x) == want == signal.find_peaks(x, height=hmin)[0].size
            # with hmin < x in place of hmin <= x the tie would lose that peak
            strict = sum(1 for a in range(1, len(x) - 1) if x[a - 1] < x[a] > x[a + 1] and hmin < x[a])
            assert strict == npk - 1


def test_special_cases_have_the_nan_patterns_they_are_named_for():
    for n in ec.N_T2:
        T2s = ec.t2_grid(n)
        got = {c[0]: metrics_ref(c, T2s) for c in [(nm, "special", f, d) for nm, f, d in ec.special_cases(n)]}
        m = got["all_zero"]
        assert np.all(np.isnan(m[[0, 1, 2, 3, 6, 7, 8]])) and m[4] == 0.0 and m[5] == 0.0
        for k, m in got.items():
            if k.startswith("inf@"):
                f = dict((nm, f) for nm, f, _ in ec.special_cases(n))[k]
                with np.errstate(all="ignore"):
                    x = f / f.sum()
                assert np.isinf(m[4]) and m[5] == 0.0 and np.isnan(x).sum() == 1 and np.all(x[~np.isnan(x)] == 0.0)
            if k.startswith("nan@"):
                assert np.isnan(m[4]) and m[5] == 0.0 and np.all(np.isnan(m[[0, 1, 6, 7, 8]]))
            if k.startswith("dist2_equals_x"):
                assert m[7] == 0.0 and m[8] == 0.0 and m[6] == 0.0
            if k.startswith("dist2_zero"):
                assert np.all(np.isfinite(m))
        # a grid wholly above cut_ie: no bin in either compartment, the T2 means are 0 / 1e-50
        m = eval_ref.voxel_metrics(np.arange(1.0, n + 1.0), ec.default_dist2(n), ec.grid_above_ie(n))
        assert np.all(m[:4] == 0.0)


def test_conditioning_gate():
    """float64 numpy agrees with long double within 1e-13 on every finite value of every case (none is left out), and so does SciPy on the
    jsd and wd of the well-conditioned ('float') cases: what the device is compared with is then known far below the device's bound"""
    pytest.importorskip("scipy")
    from scipy.spatial import distance
    from scipy.stats import wasserstein_distance
    assert np.finfo(LD).eps < 1e-18
    worst = 0.0
    for n in ec.N_T2:
        T2s = ec.t2_grid(n)
        for grid, cuts in ((T2s, (40.0, 200.0)), (T2s, ec.other_cuts(T2s)), (ec.grid_above_ie(n), (40.0, 200.0))):
            for c in ec.voxel_cases(n):
                ld, f64 = metrics_ref(c, grid, cuts, LD), metrics_ref(c, grid, cuts)
                e = ec.rel_err(f64, ld)
                assert e <= GATE, (n, c[0], e, f64, ld)
                worst = max(worst, e)
                if c[1] == "float" and grid is T2s and cuts == (40.0, 200.0):
                    x = c[2] / np.sum(c[2])
                    assert ec.rel_err([distance.jensenshannon(c[3], x), wasserstein_distance(c[3], x)], ld[7:9]) <= GATE, (n, c[0])
    print("float64 against long double: %.3g" % worst)


def test_reduce_reference_on_degenerate_columns():
    stats = pytest.importorskip("scipy.stats")
    nan_column = metrics_ref(("z", "special", np.zeros(8), ec.default_dist2(8)), ec.t2_grid(8))
    assert np.isnan(nan_column[0]) and nan_column[4] == 0.0
    for name, (pv, truth, lam, fie) in ec.degenerate_reduce_inputs(nan_column).items():
        with np.errstate(all="ignore"):
            r64 = eval_ref.reduce_metrics(pv, truth, lam, fie)
            rld = eval_ref.reduce_metrics(pv.astype(LD), truth.astype(LD), lam.astype(LD), fie.astype(LD))
        assert ec.rel_err(r64, rld) <= 1e-10, (name, r64, rld)
        if name.startswith("constant") or name == "n1" or name.startswith("nan_voxel"):
            assert np.isnan(r64[7]), (name, r64[7])               # R = 0/0 (or NaN): what pearsonr gives on a constant input
        if name.startswith("constant"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert np.isnan(stats.pearsonr(pv[0], truth[0])[0])
        if name.startswith("T_is_0"):
            assert np.isinf(r64[1]) and np.isinf(r64[4]) and np.isinf(r64[8])
        if name.startswith("T_and_M_are_0"):
            assert np.isnan(r64[1]) and np.isnan(r64[8])
        if name.startswith("T_is_1"):
            assert np.isinf(r64[8]) and np.isfinite(r64[1])
        if name.startswith("nan_voxel"):
            assert np.all(np.isnan(r64[[0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12]])) and np.isfinite(r64[9]) and np.isfinite(r64[13])


def test_midpoint_grid_puts_an_edge_on_a_fine_grid_point():
    T2s, i, j = ec.midpoint_grid()
    g = eval_ref.T2GRID[j]
    assert T2s[i - 1] + (T2s[i] - T2s[i - 1]) / 2.0 == g           # the edge between bins i - 1 and i, as rebin and the kernel compute it
    dist = np.zeros(1000)
    dist[j] = 1.0
    d2 = eval_ref.rebin(dist, T2s)
    assert d2[i] == 1.0 and d2[i - 1] == 0.0                       # >= lo, < hi: the point belongs to the upper bin


def test_sort_padding_cases_are_present():
    # 128 bins sort without padding, 127 and 65 with NaN padding behind data that hold negative numbers, zeros and a NaN of their own
    for n in (65, 127, 128):
        kinds = {c[0] for c in ec.voxel_cases(n) if c[1] == "sort"}
        assert {"sorted", "reversed", "ties", "negative", "signed_zeros", "nan_in_dist2", "x_all_equal"} <= kinds
