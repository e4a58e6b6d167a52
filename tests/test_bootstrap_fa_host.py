"""Host-side checks of the bootstrap with per-replicate flip angles and spectrum bands (no GPU): the driver's argument handling.  The
prototype of met2_fit_bootstrap_fa against its ctypes declaration is covered by test_host_logic.py, which walks every entry of SYMBOLS."""
import importlib

import numpy as np
import pytest

PKG = "multicomponent-t2-toolbox_amd"


@pytest.fixture(scope="module")
def motor():
    return importlib.import_module(PKG + ".motor")


def test_bootstrap_args_accept_the_new_keys(motor):
    assert motor._bootstrap_args(None) is None
    assert motor._bootstrap_args({}) == {"n_rep": 100, "seed": 0, "fa": "fixed", "spectrum": False}
    got = motor._bootstrap_args(dict(n_rep=8, seed=3, fa="brute-force", spectrum=1))
    assert got == {"n_rep": 8, "seed": 3, "fa": "brute-force", "spectrum": True}
    assert motor._bootstrap_args(dict(fa="spline"))["fa"] == "spline"


@pytest.mark.parametrize("bad", [dict(sed=2), dict(n_rep=8, FA="fixed"), dict(spectra=True)])
def test_bootstrap_args_reject_unknown_keys(motor, bad):
    with pytest.raises(ValueError, match="bootstrap"):
        motor._bootstrap_args(bad)


def test_bootstrap_args_reject_unknown_fa_mode(motor):
    with pytest.raises(ValueError, match="fa"):
        motor._bootstrap_args(dict(fa="smoothed"))


@pytest.mark.parametrize("fa,FA_method", [("brute-force", "brute-force"), ("spline", "spline")])
def test_replicate_fa_with_smoothing_raises_before_device_work(motor, fa, FA_method):
    # the arrays would need a GPU; the refusal comes first (no GPU on the machine that runs this test)
    d = np.ones((3, 3, 3, 32))
    m = np.ones((3, 3, 3), dtype=np.uint8)
    TE = 10.0 * np.arange(1, 33)
    with pytest.raises(ValueError, match="FA_smooth"):
        motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", FA_method, 40.0, FA_smooth="yes", bootstrap=dict(n_rep=8, seed=1, fa=fa))
    with pytest.raises(ValueError, match="FA_method"):
        motor.recon_met2_arrays(d, m, TE, 3000.0, "X2", "L2", "spline" if fa == "brute-force" else "brute-force", 40.0, FA_smooth="no",
                                bootstrap=dict(n_rep=8, seed=1, fa=fa))
    motor._bootstrap_check(motor._bootstrap_args(dict(fa="fixed")), FA_method, "yes")           # the fixed mode goes with smoothing
    motor._bootstrap_check(motor._bootstrap_args(dict(fa=fa)), FA_method, "no")


def test_quantity_names():
    plan = importlib.import_module(PKG + ".plan")
    assert plan.BOOT_QUANTITIES == plan.MAP_NAMES + ("reg",)
    assert plan.BOOT_QUANTITIES_FA == plan.BOOT_QUANTITIES + ("FA",)
    assert set(plan.BOOT_FA_MODES) == {"fixed", "brute-force", "spline"}


def test_fa_stats_in_degrees():
    plan = importlib.import_module(PKG + ".plan")
    p = plan.Met2Plan.__new__(plan.Met2Plan)                     # the conversion is host arithmetic on the stored grid
    p._h = None
    p.alpha_values = np.linspace(90.0, 180.0, 91)
    st = np.array([[10.5, 0.0], [2.0, 0.0], [3.0, 0.0], [10.0, 0.0], [90.0, 0.0]])
    deg = p.fa_stats_degrees(st)
    assert np.allclose(deg[:, 0], [100.5, 2.0, 93.0, 100.0, 180.0]) and np.allclose(deg[[0, 2, 3, 4], 1], 90.0) and deg[1, 1] == 0.0
    p.alpha_values = np.array([90.0, 100.0, 120.0, 180.0])      # not uniform: quantiles and mean interpolate, std has no image
    deg = p.fa_stats_degrees(np.array([[1.5], [0.5], [0.0], [2.0], [3.0]]))
    assert np.allclose(deg[[0, 2, 3, 4], 0], [110.0, 90.0, 120.0, 180.0]) and np.isnan(deg[1, 0])
    p.alpha_values = None
    assert p.fa_stats_degrees(st) is None
