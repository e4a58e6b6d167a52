"""Host-side checks of the label statistics (no GPU): the restatement the GPU tests compare with (tests/tools/labelstats_numpy.py) gives
np.quantile's bits on its own cases, so that its formula -- the one include/met2_hip.h states -- is the installed numpy's; the refusals of
tissue_stats in the drivers come before any device work; the two tables motor_recon_met2 writes have the documented layout and read back to
the dict; the constants of stats.py are the header's."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import labelstats_numpy as ln                                      # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"


@pytest.fixture(scope="module")
def motor():
    return importlib.import_module(PKG + ".motor")


def test_the_restatements_quantiles_are_numpys_to_the_bit():
    rng = np.random.default_rng(7)
    counts = [1, 2, 3, 7, 100, ln.SMALL_N - 1, ln.SMALL_N, ln.SMALL_N + 1, 4099, ln.CHUNK + 1]
    lab = ln.scatter_labels(rng, 30000, counts)
    v = ln.pattern_series(rng, lab, len(counts))
    offset, order = ln.member_list(lab, len(counts))
    assert list(np.diff(offset)) == counts
    q = ln.Q_TEST + (0.1, 0.9, 0.999, 1e-9)
    own, ref = ln.quantiles(v, offset, order, q), ln.quantiles_numpy(v, offset, order, q)
    assert own.shape == (len(counts), len(ln.PATTERNS), len(q))
    assert np.array_equal(own, ref, equal_nan=True)
    assert np.array_equal(np.isnan(own), np.isnan(ref))
    # the voxel-major view of the same numbers
    assert np.array_equal(ln.quantiles(np.ascontiguousarray(v.T), offset, order, q, "voxel"), own, equal_nan=True)


def test_the_restatements_member_list_and_moments():
    lab = np.array([2, -1, 0, 3, 2, 0, 2, 7], dtype=np.int32)
    offset, order = ln.member_list(lab, 3)
    assert offset.tolist() == [0, 2, 2, 5] and order.tolist() == [2, 5, 0, 4, 6]
    v = np.array([[1.0, 9.0, 2.0, 9.0, np.nan, 4.0, 3.0, 9.0]])
    m = ln.moments(v, offset, order)
    assert m[0, 0].tolist() == [2.0, 3.0, np.sqrt(np.longdouble(2.0))] and np.isnan(m[1, 0, 1:]).all() and m[1, 0, 0] == 0
    assert m[2, 0, 0] == 2 and m[2, 0, 1] == 2.0                     # the NaN is skipped
    assert np.array_equal(ln.quantiles(v, offset, order, (0.5,))[:, 0, 0], [3.0, np.nan, 2.0], equal_nan=True)


def test_tissue_stats_is_refused_before_any_device_work(motor):
    chk = motor._tissue_stats_check
    assert chk("no", "no", False) is False and chk("no", "no", True) is False
    assert chk("yes", "yes", False) is True and chk("yes", "pve", False, 0.5) is True
    with pytest.raises(ValueError, match="tissue_stats must be"):
        chk("maybe", "pve", False)
    with pytest.raises(ValueError, match="needs segment"):
        chk("yes", "no", False)
    with pytest.raises(ValueError, match="distributed"):
        chk("yes", "pve", True)
    for bad in (0.49, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="pve_threshold"):
            chk("yes", "pve", False, bad)
    # the drivers raise it from the arguments alone: there is no GPU on the machine that runs this test
    d = np.ones((3, 3, 3, 32))
    m = np.ones((3, 3, 3), dtype=np.uint8)
    TE = 10.0 * np.arange(1, 33)
    with pytest.raises(ValueError, match="needs segment"):
        motor.recon_met2_arrays(d, m, TE, 3000.0, tissue_stats="yes")
    with pytest.raises(ValueError, match="tissue_stats must be"):
        motor.recon_met2_arrays(d, m, TE, 3000.0, bias_correct="yes", voxel_size=(1, 1, 1), segment="pve", tissue_stats="on")
    with pytest.raises(ValueError, match="pve_threshold"):
        motor.recon_met2_arrays(d, m, TE, 3000.0, bias_correct="yes", voxel_size=(1, 1, 1), segment="pve", tissue_stats="yes", pve_threshold=0.3)


def canned(rng, L=2, n_t2=5, n_q=5):
    ts = {"labels": np.array([1, 3][:L]), "quantities": motor_quantities(), "q": np.array([0.025, 0.25, 0.5, 0.75, 0.975][:n_q]),
          "n": rng.integers(1, 99, (L, 8)).astype(np.float64), "mean": rng.standard_normal((L, 8)), "std": rng.random((L, 8)),
          "quantiles": rng.standard_normal((L, 8, n_q)), "spectrum_mean": rng.random((L, n_t2)), "spectrum_quantiles": rng.random((L, n_t2, n_q)),
          "T2s": np.logspace(1, 3, n_t2), "mean_signal_fsol": rng.random((L + 1, n_t2))}
    ts["all"] = {"n": rng.integers(1, 99, 8).astype(np.float64), "mean": rng.standard_normal(8), "std": rng.random(8),
                 "quantiles": rng.standard_normal((8, n_q)), "spectrum_mean": rng.random(n_t2), "spectrum_quantiles": rng.random((n_t2, n_q))}
    ts["mean"][1, 2] = np.nan
    return ts


def motor_quantities():
    return importlib.import_module(PKG + ".motor").STAT_QUANTITIES


def test_the_tables_have_the_documented_layout_and_read_back(motor, tmp_path):
    assert motor.STAT_QUANTITIES == ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC", "FA", "reg_param")
    ts = canned(np.random.default_rng(3))
    table, spectra = motor.tissue_stats_tables(ts)
    assert table.shape == (3 * 8, 5 + 5) and spectra.shape == (1 + 2 * 3, 5)
    np.savetxt(str(tmp_path / "s.csv"), table, delimiter=",", fmt="%s")
    np.savetxt(str(tmp_path / "p.csv"), spectra, delimiter=",", fmt="%s")
    rows = [line.split(",") for line in open(str(tmp_path / "s.csv")).read().split()]
    assert [r[0] for r in rows] == ["1"] * 8 + ["3"] * 8 + ["all"] * 8
    assert [r[1] for r in rows] == list(motor.STAT_QUANTITIES) * 3
    num = np.array([[float(x) for x in r[2:]] for r in rows])
    for i in range(3):
        src = ts["all"] if i == 2 else {k: ts[k][i] for k in motor.STAT_KEYS}
        want = np.column_stack([src["n"], src["mean"], src["std"], src["quantiles"]])
        assert np.array_equal(num[8 * i:8 * i + 8], want, equal_nan=True)          # repr round-trips a double
    back = np.loadtxt(str(tmp_path / "p.csv"), delimiter=",")
    assert np.array_equal(back[0], ts["T2s"])
    assert np.array_equal(back[1::2], np.vstack([ts["spectrum_mean"], ts["all"]["spectrum_mean"]]))
    assert np.array_equal(back[2::2], ts["mean_signal_fsol"])


def test_the_constants_are_the_headers():
    stats = importlib.import_module(PKG + ".stats")
    text = open(os.path.join(ROOT, "include", "met2_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define MET2_STATS_(\w+) (\d+)", text)}
    assert got == {"CHUNK": stats.CHUNK, "SMALL_N": stats.SMALL_N, "MAX_LABEL": stats.MAX_LABEL, "MAX_SERIES": stats.MAX_SERIES, "MAX_Q": stats.MAX_Q}
    assert stats.MAX_LABEL >= 1024 and stats.MAX_SERIES >= 4096 and stats.MAX_Q >= 16
    assert (ln.CHUNK, ln.SMALL_N) == (stats.CHUNK, stats.SMALL_N) and stats.DEFAULT_Q == (0.025, 0.25, 0.5, 0.75, 0.975)
