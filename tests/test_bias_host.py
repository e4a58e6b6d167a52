"""The numpy restatement of the bias-field estimation (tests/tools/bias_numpy.py, the reference of tests/test_gpu_bias.py) and its test
volumes, checked on the CPU so that the GPU tests cannot hide behind them: a known answer, how far rounding moves the result, how far
the initialisation is from depending on one sample, the smoothing weights, the degenerate volumes."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import bias_numpy as bn                                            # noqa: E402


@functools.lru_cache(maxsize=None)
def run(name, dtype="float64"):
    v, mask, vox, kw = bn.case(name)
    return bn.bias_field(v, mask, vox, dtype=np.dtype(dtype).type, **kw)


def test_known_answer_on_the_phantom():
    """Three concentric classes (discs of radius 0.35 and 0.65, mask 0.9 of the half-width) at 500 / 800 / 1100 under
    exp(0.25 x - 0.2 y + 0.15 x y + 0.1 z) (rms 0.159 on the mask) with 2 % noise, n_outer = 8.  Measured with this restatement:
    correlation of the estimated with the true log field on Omega 0.8078 (0.8278 at n_outer = 4), residual rms 0.0976; coefficient of
    variation per class 0.0860 / 0.1351 / 0.1855 before and 0.0206 / 0.0421 / 0.1256 after, at a noise floor of 0.02.  That is short of
    the 0.9966 and 0.020-0.024 first reported for a phantom of this description: with concentric classes the field's radial part cannot
    be told from the class contrast, and the outer ring, which meets the mask's edge, keeps a third of its spread (other radii and
    orders of the levels gave correlations between 0.37 and 0.98).  The bounds leave a tenth of the distance to the uncorrected values
    (correlation 0 for no field at all)."""
    v, mask, logf, lab = bn.phantom(seed=bn.SEEDS["phantom"])
    res = bn.bias_field(v, mask, (2.0, 2.0, 4.0), n_outer=8)
    om = res["omega"]
    est, true = res["b"][om], logf[om] - logf[om].mean()
    corr = float(np.corrcoef(est, true)[0, 1])
    rms = float(np.sqrt(np.mean((est - est.mean() - true) ** 2)))
    cv = lambda a, k: float(a[om & (lab == k)].std() / a[om & (lab == k)].mean())
    before, after = [cv(v, k) for k in range(3)], [cv(res["out"], k) for k in range(3)]
    print("correlation %.4f, residual rms %.4f of %.4f, cv before %s after %s" % (corr, rms, float(true.std()), before, after))
    assert corr >= 0.8078 - 0.1 * 0.8078
    assert rms <= 0.0976 + 0.1 * (float(true.std()) - 0.0976)
    for k, floor in enumerate((0.0206, 0.0421, 0.1256)):
        assert after[k] <= floor + 0.1 * (before[k] - floor), k


@pytest.mark.parametrize("name", bn.CASES)
def test_rounding_does_not_move_the_field(name):
    """fp64 against longdouble: max |field / field_ld - 1| over the committed cases is 1.2e-13 (k8floor; 2.7e-14 on coarse, 4e-15 on the phantom), which is
    what allows the GPU tests to ask for 1e-9."""
    a, b = run(name), run(name, "longdouble")
    rel = float(np.abs(a["field"] / b["field"] - 1.0).max())
    print(name, "%.3e" % rel)
    assert rel <= 1e-12
    assert np.array_equal(a["support"], b["support"]) and np.array_equal(a["omega"], b["omega"])


@pytest.mark.parametrize("name", bn.CASES)
def test_initialisation_does_not_hang_on_one_sample(name):
    v, mask, vox, kw = bn.case(name)
    margins = bn.init_margin(v, mask, kw.get("n_class", 3))
    print(name, margins)
    assert len(margins) == kw.get("n_class", 3)
    assert min(min(m) for m in margins) >= 2


def test_a_wrong_initial_mean_shows():
    worst = 0.0
    for name in bn.CASES:
        v, mask, vox, kw = bn.case(name)
        if kw.get("n_outer", 4) == 0:
            continue
        ref = run(name)["field"]
        for k in range(kw.get("n_class", 3)):
            moved = bn.bias_field(v, mask, vox, init_shift=(k, 1), **kw)["field"]
            worst = max(worst, float(np.abs(moved / ref - 1.0).max()))
    print("one bin in one initial mean moves the field by up to %.3e" % worst)
    assert worst > 1e-6


def test_radius_and_weights_follow_gaussian_filter1d():
    ndi = pytest.importorskip("scipy.ndimage")
    for fwhm, d in ((20.0, 2.0), (20.0, 4.0), (20.0, 1.0), (20.0, 1.25), (20.0, 40.0), (20.0, 80.0), (7.0, 3.0)):
        r, w = bn.radius_weights(fwhm, d)
        sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0))) / d
        assert r == int(4.0 * sigma + 0.5) and w.shape == (2 * r + 1,) and abs(w.sum() - 1.0) < 1e-15
        line = np.zeros(4 * r + 9)
        line[2 * r + 4] = 1.0
        want = ndi.gaussian_filter1d(line, sigma, mode="constant", cval=0.0, truncate=4.0)
        got = bn.smooth_axis(line[:, None, None], w, 0)[:, 0, 0]
        assert np.count_nonzero(want) == 2 * r + 1
        assert np.abs(got - want).max() <= 1e-15
    assert bn.radius_weights(20.0, 1.0)[0] == 34 and bn.radius_weights(20.0, 80.0)[0] == 0 and bn.radius_weights(20.0, 40.0)[0] == 1
    # zero extension, no reflection: a constant line falls off towards its ends
    r, w = bn.radius_weights(20.0, 4.0)
    s = bn.smooth_axis(np.ones((5, 1, 1)), w, 0)[:, 0, 0]
    assert s[2] < 1.0 and s[0] < s[2] and np.allclose(s, s[::-1])


def test_cases_are_what_they_say():
    radii = lambda vox: tuple(bn.radius_weights(20.0, d)[0] for d in vox)
    v, mask, vox, kw = bn.case("phantom")
    assert v.shape == (40, 36, 12) and vox == (2.0, 2.0, 4.0) and radii(vox) == (17, 17, 8)
    v, mask, vox, kw = bn.case("thin")
    assert v.shape == (33, 5, 1) and radii(vox) == (34, 34, 34)
    v, mask, vox, kw = bn.case("wave")
    assert v.shape == (65, 3, 7) and len(set(radii(vox))) == 3
    assert bn.case("coarse")[0].shape == (9, 9, 9) and bn.case("coarse")[2] == (40.0, 40.0, 40.0) and radii(bn.case("coarse80")[2]) == (0, 0, 0)
    # coarse80: smoothing is the identity, so b moves by the raw ratio R / W on Omega and the support is Omega itself
    r80 = run("coarse80")
    assert np.array_equal(r80["support"], r80["omega"]) and np.all(r80["field"][~r80["omega"]] == 1.0)
    # holes: non-positive and non-finite voxels inside the mask, and a support that leaves part of the volume out
    v, mask, vox, kw = bn.case("holes")
    inside = mask != 0
    assert (v[inside] == 0).any() and (v[inside] < 0).any() and np.isnan(v[inside]).any() and np.isinf(v[inside]).any()
    res = run("holes")
    assert not res["support"].all() and np.all(res["field"][~res["support"]] == 1.0) and (res["field"][res["support"]] != 1.0).any()
    assert np.array_equal(np.isnan(res["out"]), np.isnan(v)) and np.array_equal(np.isinf(res["out"]), np.isinf(v))
    assert res["omega"].sum() == inside.sum() - 5
    assert bn.case("k1")[3] == {"n_class": 1} and bn.case("k8")[3] == {"n_class": 8} and bn.case("outer0")[3] == {"n_outer": 0}


def test_a_class_reaches_the_variance_floor():
    """The phantom's classes cannot: the log of 2 % multiplicative noise has variance 4e-4, and with K = 8 the smallest class variance over
    80 seeds of the phantom was 5.5e-4 and the smallest class weight 590 voxels.  Where the smoothing is (nearly) the identity the field
    takes the residual up and classes do collapse: 'coarse', 'coarse80' and 'k8floor' (the coarse volume with K = 8) end with classes at
    the floor of 1e-6."""
    for name in ("coarse", "coarse80", "k8floor"):
        v, mask, vox, kw = bn.case(name)
        trace = []
        res = bn.bias_field(v, mask, vox, trace=trace, **kw)
        K = kw.get("n_class", 3)
        assert (res["classes"][K:2 * K] == bn.VAR_FLOOR).any() or min(s.min() for _, _, s, _ in trace) == 0, name
    v, mask, vox, kw = bn.case("k8")
    trace = []
    bn.bias_field(v, mask, vox, trace=trace, **kw)
    assert min(var.min() for _, _, _, var in trace) > 1e-4               # see the docstring


def test_degenerate_volumes_give_a_unit_field():
    v, mask, vox, _ = bn.case("phantom")
    for vol, m, mu in ((v, np.zeros_like(mask), 0.0), (np.full(v.shape, 750.0), mask, np.log(750.0)), (-v, None, 0.0)):
        res = bn.bias_field(vol, m, vox)
        assert np.all(res["field"] == 1.0) and np.array_equal(res["out"], vol)
        assert np.array_equal(res["classes"], np.concatenate([np.full(3, mu), np.zeros(3), np.full(3, 1.0 / 3.0)]))


def test_outer0_keeps_the_initial_classes():
    v, mask, vox, kw = bn.case("outer0")
    res = run("outer0")
    assert np.all(res["field"] == 1.0) and np.array_equal(res["out"], v)
    y = np.log(v[mask != 0])
    assert np.allclose(res["classes"][3:6], y.var() / 9.0, rtol=1e-14) and np.all(res["classes"][6:] == 1.0 / 3.0)
    assert np.all(np.diff(res["classes"][:3]) > 0) and y.min() < res["classes"][0] and res["classes"][2] < y.max()
