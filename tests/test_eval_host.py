"""CPU tests of the Monte-Carlo study (met2_amd.evaluate): the numpy restatement tests/eval_ref.py against SciPy on adversarial spectra
(the GPU kernels are checked against eval_ref in test_gpu_evaluate.py), and the table writer against the reference's committed tables."""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import eval_ref
from conftest import GOLDEN

PKG = "multicomponent-t2-toolbox_amd"


def fixture():
    with open(os.path.join(GOLDEN, "eval_tables_paper.json")) as f:
        return json.load(f)


def adversarial_spectra():
    rng = np.random.default_rng(5)
    xs = [
        np.array([0.0, 1.0, 1.0, 1.0, 0.0, 2.0, 2.0, 0.5, 0.0, 0.0]),          # plateaus
        np.array([0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]),          # a single non-zero
        np.array([5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0]),          # endpoints only: never peaks
        np.array([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]),          # a plateau that runs into the last sample
        np.array([0.0, 1e-5, 0.0, 1.0, 0.0, 0.99999e-5, 0.0, 0.0, 2e-5, 1e-5]), # ties at the height threshold 1e-5 max
        np.array([0.0, 2.0, 1.0, 2.0, 1.0, 2.0, 2.0, 1.0, 3.0, 3.0]),
    ]
    for _ in range(6):                                                         # sparse NNLS-like spectra with runs of exact zeros
        x = np.where(rng.random(60) < 0.2, rng.random(60), 0.0)
        x[rng.integers(0, 60, 3)] = 0.5                                        # exact ties
        xs.append(x)
    xs.append(np.exp(-0.5 * ((np.arange(120) - 40.0) / 6.0) ** 2))           # smooth, 120 bins
    return xs


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
