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
    """fp64 against longdouble: max |field / field_ld - 1| over the committed cases is 1.5e-13 (big; 1.2e-13 on k8floor, 8.3e-14 on bigall, 2.7e-14 on
    coarse, 4e-15 on the phantom, 3.5e-15 on seams, 1.8e-15 on r64), which is what allows the GPU tests to ask for 1e-9."""
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
    # the cases that reach the tile seams of the smoothing and the second-stage sums' stride: shapes, radii, chunks of 1024
    chunks = lambda n: -(-int(n) // 1024)
    v, mask, vox, kw = bn.case("seams")
    assert v.shape == (9, 70, 131) and vox == (8.0, 3.0, 2.0) and radii(vox) == (4, 11, 17) and kw == {}
    assert v.shape[1] > 64 and v.shape[2] > 128 and int(bn.domain(v, mask).sum()) == 46374
    v, mask, vox, kw = bn.case("r64")
    assert v.shape == (130, 20, 3) and vox == (0.53, 2.0, 4.0) and radii(vox) == (64, 17, 8) and int(bn.domain(v, mask).sum()) == 4668
    v, mask, vox, kw = bn.case("big")
    assert v.shape == (64, 64, 65) and radii(vox) == (4, 4, 4) and chunks(v.size) == 260 and int(bn.domain(v, mask).sum()) == 163280
    assert not run("big")["support"].all()
    v, mask, vox, kw = bn.case("bigall")
    assert v.shape == (64, 64, 65) and mask is None and radii(vox) == (4, 4, 4) and chunks(bn.domain(v, mask).sum()) == 260
    assert np.array_equal(v, bn.case("big")[0])


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


@pytest.mark.parametrize("name", bn.CASES)
def test_the_composed_restatement_returns_the_bits_of_the_old_body(name):
    """bias_field() is composed of the stage functions the stage tests use; _bias_field_v0 is its body from before that"""
    v, mask, vox, kw = bn.case(name)
    new, old = run(name), bn._bias_field_v0(v, mask, vox, **kw)
    assert sorted(new) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k], equal_nan=True), k
    if name == "k8floor":
        tn, to = [], []
        bn.bias_field(v, mask, vox, trace=tn, init_shift=(1, 1), **kw)
        bn._bias_field_v0(v, mask, vox, trace=to, init_shift=(1, 1), **kw)
        assert len(tn) == len(to) and all(np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) for a, b in zip(tn, to))


# The stage tests on the device (tests/test_gpu_bias_stages.py) ask for 1e-12 of a scale each; that is fair only if the formula itself,
# evaluated in fp64 by the restatement, stays well inside it on the same inputs.  Below: every committed stage input, fp64 against long
# double, in the scale the device test uses, within 1e-13.
LD = np.longdouble


def test_stage_inputs_domain_and_init_within_1e_13():
    for name in bn.DOMAIN_INPUTS:
        v, mask = bn.domain_input(name)
        y, om = bn.log_domain(v, mask)
        yl, oml = bn.log_domain(v, mask, LD)
        assert np.array_equal(om, oml) and np.all(y[~om] == 0)
        assert float((np.abs(y - yl) / np.maximum(1.0, np.abs(yl))).max()) <= 1e-13, name
    for name in bn.INIT_INPUTS:
        v, mask, K = bn.init_input(name)
        y, om = bn.log_domain(v, mask)
        a, b = bn.init_classes(y[om], K), bn.init_classes(y[om], K, LD)
        assert a["degenerate"] == b["degenerate"] == (name in ("n1", "const")), name
        assert a["lo"] == b["lo"] and a["hi"] == b["hi"]
        if a["degenerate"]:
            assert np.all(a["mu"] == a["lo"]) and np.all(a["var"] == 0) and np.all(a["pi"] == 1.0 / K)
            continue
        assert abs(a["mean"] - b["mean"]) <= 1e-13 * float(np.abs(y[om]).mean()), name
        assert abs(a["ss"] - b["ss"]) <= 1e-13 * float(b["ss"]), name
        assert float(np.abs(a["var"] / b["var"] - 1.0).max()) <= 1e-13, name
        # the bins of the initial means must not hang on the rounding of one bin expression: the same in long double
        assert a["jk"] == b["jk"] and float(np.abs(a["mu"] / b["mu"] - 1.0).max()) <= 1e-13, name


@pytest.mark.parametrize("name", bn.EM_INPUTS)
def test_stage_inputs_em_within_1e_13(name):
    d = bn.em_input(name)
    y, om = bn.log_domain(d["v"], d["mask"])
    idx = np.flatnonzero(om)
    classes = d["classes"]
    for step in range(2 if name == "dying" else 1):
        a, b = bn.em_reference(y, d["b"], idx, *classes, dtype=np.float64), bn.em_reference(y, d["b"], idx, *classes)
        amp = 1.0 + b["lmax"] if d["floor"] else 1.0
        live = b["sums_abs"] > 0
        assert np.array_equal(a["sums"][~live], b["sums"][~live])
        fig = {"sums": float((np.abs(a["sums"] - b["sums"])[live] / b["sums_abs"][live]).max()),
               "R": float((np.abs(a["R"] - b["R"]) / b["R_abs"]).max()), "W": float((np.abs(a["W"] - b["W"]) / b["W_abs"]).max())}
        (mu, var, pi), (mul, varl, pil) = a["classes"], b["classes"]
        spread = b["sums"][2][live[0]] / b["sums"][0][live[0]] + (mul - np.asarray(classes[0]))[live[0]] ** 2
        fig["mu"] = float(np.abs(mu / mul - 1.0).max())
        fig["var"] = float((np.abs(var - varl)[live[0]] / spread).max())
        fig["pi"] = float(np.abs(pi - pil).max())
        print(name, step, "lmax %.3g" % b["lmax"], fig)
        assert max(fig.values()) <= 1e-13 * amp, (name, fig)
        if name == "dying":
            assert a["sums"][0][2] == 0 and pi[2] == 0 and mu[2] == classes[0][2] and var[2] == classes[1][2]
            assert all(np.isfinite(x).all() for x in (a["sums"], a["R"], a["W"], mu, var, pi))
        classes = a["classes"]
    if name == "floor":
        assert b["lmax"] > 1e3


def test_stage_inputs_smooth_and_update_within_1e_13():
    for name in bn.SMOOTH_INPUTS:
        a, radii, weights, axis = bn.smooth_input(name)
        (x, _), (xl, mag) = bn.smooth_reference(a, radii, weights, axis, np.float64), bn.smooth_reference(a, radii, weights, axis)
        assert float((np.abs(x - xl) / mag).max()) <= 1e-13, name
        assert not np.array_equal(a[..., 0], a[..., 1]) and all(not np.allclose(w, w[::-1]) for w in weights if w.size > 1)
    for name in bn.UPDATE_INPUTS:
        b, S, idx = bn.update_input(name)
        (nb, bm, _), (nbl, bml, scale) = bn.update_reference(b, S, idx, np.float64), bn.update_reference(b, S, idx)
        D = S[..., 1] > 0
        assert not D.all() and D.reshape(-1)[idx].all() and idx.size < D.sum()          # the support is larger than the domain
        assert np.array_equal(nb[~D], b[~D])
        assert abs(bm - bml) <= 1e-13 * float(np.abs(b).mean() + np.abs(S[..., 0][D] / S[..., 1][D]).mean()), name
        assert float((np.abs(nb - nbl)[D] / scale[D]).max()) <= 1e-13, name


def test_the_reviving_class_input_does_what_it_says():
    """bias_numpy.revive_input: the third class dies in the first step (s = 0 exactly), stays dead under the header's rule, and would get a
    posterior far above the underflow threshold in the second step if its log coefficient were left finite"""
    yv, (mu, var, pi) = bn.revive_input()
    u = yv.reshape(-1)
    mu, var, pi = mu.copy(), var.copy(), pi.copy()
    lc3 = np.log(pi[2]) - 0.5 * np.log(var[2])
    l = bn.log_terms(u, mu, var, pi)
    gap = (l[2] - l.max(axis=0)).max()
    assert -1400 < gap < -1000                                          # exp() gives exactly 0 below -745.2
    s = bn.m_step(bn.e_step(u, mu, var, pi), u, mu, var, pi)
    assert s[2] == 0 and pi[2] == 0 and mu[2] == 9.5237 and var[2] == 1e-3
    l = bn.log_terms(u, mu, var, pi)
    assert np.all(l[2] == -np.inf)
    kept = lc3 - (u - mu[2]) ** 2 / (2.0 * var[2])                      # the exponent with the coefficient of before the class died
    gap = (kept - l[:2].max(axis=0)).max()
    assert -500 < gap < -100 and np.exp(gap) > 1e-200
    s = bn.m_step(bn.e_step(u, mu, var, pi), u, mu, var, pi)
    assert s[2] == 0 and pi[2] == 0 and np.isfinite(mu).all() and np.isfinite(var).all() and abs(pi.sum() - 1.0) < 1e-15
