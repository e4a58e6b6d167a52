"""The kernels of the bias-field correction stage by stage (csrc/met2_bias.hip through met2_bias_domain, met2_bias_init, met2_bias_em,
met2_bias_smooth, met2_bias_update, met2_bias_apply; bias.py), each on the DEVICE's output of the stage before it, against the long-double
evaluation of the formula include/met2_hip.h states (tests/tools/bias_numpy.py) on that same input.

The bar is 1e-12 of a scale named per stage (the project's stage bar: Gibbs stages, BET statistics): about four orders above what fp64
delivers and three below the 1e-9 of tests/test_gpu_bias.py, behind which a stage that is wrong at 1e-11 or a tap of weight 1.5e-5 in the
wrong place could hide.  It is a condition on the inputs, not a measurement: tests/test_bias_host.py shows that on every input used here
the fp64 restatement stays within 1e-13 of the long-double one.  What is integer or a single correctly rounded operation is compared
bit for bit: the compacted list, lo, hi, the histogram, the bins of the initial means, zeros off the domain, the impulse responses.

Shapes (bias_numpy.*_input): volumes that are no multiple of 4 or of a chunk of 1024 and an exact multiple, chunks without a domain voxel,
lists of 1024 k, 1024 k + 1 and 1 entries, 260 chunks and 260 partials (the scan's second pass, the second-stage sums' stride), tile seams
of the smoothing on every axis with radii 0, 1, 17, 63 and 64, a class that dies and a class at the variance floor.

Measured on an MI355X (profiles/bias_parity.json, written through MET2_BIAS_PARITY_JSON): log 7.3e-17; init 3e-17 to 2.5e-16; the sums of an EM
step 1.0e-16 to 1.9e-16, a chunk's partials up to 3.7e-14, the class update up to 2.0e-15; R 1.5e-15, W 1.2e-15; smoothing 7.8e-17 to 3.6e-16;
update 3.1e-16; the host's weights 4.2e-17.  Each of twelve value-only mutations of the kernels fails one of these tests."""
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
import bias_numpy as bn                                            # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
LD = np.longdouble
BAR = 1e-12


def record(name, figures):
    """with MET2_BIAS_PARITY_JSON set, the measured deviations are kept in that file (profiles/bias_parity.json was written this way)"""
    path = os.environ.get("MET2_BIAS_PARITY_JSON")
    print(name, figures)
    if not path:
        return
    table = json.load(open(path)) if os.path.exists(path) else {}
    table["stage " + name] = figures
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def bias():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".bias")


@functools.lru_cache(maxsize=None)
def device_domain(kind, name):
    """the device's y and idx of a committed input, computed once and shared, never written to"""
    mod = importlib.import_module(PKG + ".bias")
    d = {"domain": lambda: bn.domain_input(name), "init": lambda: bn.init_input(name)[:2],
         "em": lambda: (bn.em_input(name)["v"], bn.em_input(name)["mask"])}[kind]()
    y, idx = mod.bias_domain(*d)
    y.setflags(write=False)
    idx.setflags(write=False)
    return d[0], d[1], y, idx


@pytest.mark.parametrize("name", bn.DOMAIN_INPUTS)
def test_domain(bias, name):
    """idx is Omega in memory order exactly, y is 0 off Omega and within 1e-12 max(1, |log v|) of the long-double log on it"""
    v, mask, y, idx = device_domain("domain", name)
    om = bn.domain(v, mask)
    assert idx.dtype == np.int32 and np.array_equal(idx, np.flatnonzero(om))
    assert y.shape == v.shape and np.all(y[~om] == 0.0) and not np.signbit(y[~om]).any()
    ref = np.log(v[om].astype(LD))
    err = float((np.abs(y[om] - ref) / np.maximum(1.0, np.abs(ref))).max())
    record("domain " + name, {"n": int(v.size), "N": int(idx.size), "log_rel": err})
    assert err <= BAR
    if name == "gap":
        assert not om.reshape(-1)[2048:4096].any()                     # two whole chunks without a domain voxel
    if name == "exact":
        assert v.size % 1024 == 0
    if name == "odd":
        assert v.size % 4 and v.size % 1024
    if name == "scan2":
        assert -(-v.size // 1024) == 260
    if name == "bad":
        inside = mask != 0
        assert np.isnan(v[inside]).any() and np.isinf(v[inside]).any() and (v[inside] == 0).any() and (v[inside] < 0).any()


def test_domain_tensor_face_and_empty_domain(bias):
    v, mask, y, idx = device_domain("domain", "odd")
    ty, tidx = bias.bias_domain(torch.as_tensor(v, device="cuda"), torch.as_tensor(mask, device="cuda"))
    assert torch.is_tensor(ty) and ty.is_cuda and np.array_equal(ty.cpu().numpy(), y) and np.array_equal(tidx.cpu().numpy(), idx)
    y0, idx0 = bias.bias_domain(v, np.zeros_like(mask))
    assert idx0.size == 0 and np.all(y0 == 0.0)
    y1, idx1 = bias.bias_domain(-v, None)
    assert idx1.size == 0 and np.all(y1 == 0.0)


@pytest.mark.parametrize("name", bn.INIT_INPUTS)
def test_init(bias, name):
    """lo, hi, the histogram and the bins j_k of the initial means equal the fp64 restatement's on the device's y bit for bit (the bin
    expression is correctly rounded fp64 on both sides); the mean within 1e-12 mean|y|, every chunk's partial of sum (y - mean)^2 within
    1e-12 of itself (its terms are positive), the variance and the means within 1e-12 relative"""
    K = bn.init_input(name)[2]
    v, mask, y, idx = device_domain("init", name)
    got = bias.bias_init(y, idx, K)
    yl = y.reshape(-1)[idx]
    ref64, ref = bn.init_classes(yl, K), bn.init_classes(yl, K, LD)
    assert got["degenerate"] == ref64["degenerate"] == (name in ("n1", "const"))
    assert got["lo"] == ref64["lo"] and got["hi"] == ref64["hi"]
    mu, var, pi = got["classes"].reshape(3, K)
    if got["degenerate"]:                                              # the header's degenerate classes
        assert got["lo"] == got["hi"] == yl[0] and np.all(mu == got["lo"]) and np.all(var == 0.0) and np.all(pi == 1.0 / K)
        assert not got["hist"].any() and got["ss_part"] is None
        return
    assert idx.size == {"n2048": 2048, "n2049": 2049}.get(name, 266240)
    assert np.array_equal(got["hist"].astype(np.int64), ref64["hist"]) and int(got["hist"].sum()) == idx.size
    width = (ref["hi"] - ref["lo"]) / LD(bn.NBINS)
    jk = np.rint(((mu.astype(LD) - ref["lo"]) / width - LD(0.5)).astype(np.float64)).astype(np.int64)
    e_mean = float(abs(got["mean"] - ref["mean"]) / np.abs(yl).mean())
    part = got["ss_part"]
    assert part.shape == (-(-idx.size // 1024),)
    d2 = (yl.astype(LD) - LD(got["mean"])) ** 2                         # about the DEVICE's mean, which stat2 ran with
    want = np.array([d2[c:c + 1024].sum() for c in range(0, idx.size, 1024)])
    e_part = float((np.abs(part - want) / want).max())
    ss = LD(importlib.import_module(PKG + ".bias").partial_sum(part))   # the sum bias_init_kernel takes, in its order
    e_var = float(np.abs(var / (ss / LD(idx.size) / LD(K * K)) - 1.0).max())
    e_var_ld = float(np.abs(var / ref["var"] - 1.0).max())
    e_mu = float(np.abs(mu / ref["mu"] - 1.0).max())
    record("init " + name, {"N": int(idx.size), "K": K, "mean_rel": e_mean, "ss_part_rel": e_part, "var_of_device_sum_rel": e_var,
                            "var_rel": e_var_ld, "mu_rel": e_mu})
    assert jk.tolist() == ref64["jk"] == ref["jk"]
    assert e_mean <= BAR and e_part <= BAR and e_var <= BAR and e_var_ld <= BAR and e_mu <= BAR
    assert np.all(pi == 1.0 / K) and np.all(var == var[0])


def em_compare(name, step, y, b, idx, classes, got, floor):
    """got: bias_em(.., n_em = 1, want_rw = True) on `classes` -> the new classes; the figures are asserted within BAR, or within
    BAR (1 + max |l_k|) of the long-double run where a class sits at the variance floor"""
    K = len(classes[0])
    ref = bn.em_reference(y, b, idx, *classes)
    npart = -(-idx.size // 1024)
    assert got["part"].shape == (3, K, npart) and got["sums"].shape == (3, K)
    live = ref["sums_abs"] > 0
    assert np.all(got["sums"][~live] == 0.0)
    fig = {"N": int(idx.size), "K": K, "lmax": ref["lmax"],
           "sums_rel": float((np.abs(got["sums"] - ref["sums"])[live] / ref["sums_abs"][live]).max())}
    # every chunk's partial against the long-double sum over that chunk of the list
    u = (y.reshape(-1)[idx] - np.asarray(b).reshape(-1)[idx]).astype(LD)
    mu0, var0, pi0 = (np.asarray(a).astype(LD) for a in classes)
    p = bn.e_step(u, mu0, var0, pi0)
    worst = 0.0
    for c in range(npart):
        sl = slice(1024 * c, 1024 * (c + 1))
        s, sa = bn.em_sums(p[:, sl], u[sl], mu0)
        ok = sa > 0
        assert np.all(got["part"][:, :, c][~ok] == 0.0)
        if ok.any():
            worst = max(worst, float((np.abs(got["part"][:, :, c] - s)[ok] / sa[ok]).max()))
    fig["part_rel"] = worst
    # the class update: the header's formula on the DEVICE's sums
    mu, var, pi = got["classes"].reshape(3, K)
    mul, varl, pil = bn.class_update(got["sums"].astype(LD), mu0, var0, pi0, idx.size)
    alive = got["sums"][0] > 0
    spread = (got["sums"][2][alive] / got["sums"][0][alive]).astype(LD) + (mul - mu0)[alive] ** 2
    fig["mu_rel"] = float(np.abs(mu / mul - 1.0).max())
    fig["var_of_spread"] = float((np.abs(var - varl)[alive] / spread).max()) if alive.any() else 0.0
    fig["pi_abs"] = float(np.abs(pi - pil).max())
    assert np.array_equal(mu[~alive], np.asarray(classes[0])[~alive]) and np.array_equal(var[~alive], np.asarray(classes[1])[~alive])
    assert np.all(pi[~alive] == 0.0)
    assert np.all(var >= bn.VAR_FLOOR)
    # R, W of the final E-step, which ran with the classes AFTER the step
    rw = got["rw"].reshape(-1, 2)
    off = np.ones(rw.shape[0], dtype=bool)
    off[idx] = False
    assert np.all(rw[off] == 0.0)
    ref2 = bn.em_reference(y, b, idx, mu, var, pi)
    fig["R_rel"] = float((np.abs(rw[idx, 0] - ref2["R"]) / ref2["R_abs"]).max())
    fig["W_rel"] = float((np.abs(rw[idx, 1] - ref2["W"]) / ref2["W_abs"]).max())
    fig["lmax_after"] = ref2["lmax"]
    record("em %s step %d" % (name, step), fig)
    assert np.isfinite(got["part"]).all() and np.isfinite(got["classes"]).all() and np.isfinite(rw).all()
    amp = 1.0 + max(ref["lmax"], ref2["lmax"]) if floor else 1.0
    for k in ("sums_rel", "part_rel", "mu_rel", "var_of_spread", "pi_abs", "R_rel", "W_rel"):
        assert fig[k] <= BAR * amp, (k, fig)
    return got["classes"].reshape(3, K)


@pytest.mark.parametrize("name", bn.EM_INPUTS)
def test_em_step_and_residual(bias, name):
    """One EM step, then R and W, on the device's y.  The 3 K sums and every chunk's partials within 1e-12 of sum |terms|; the new classes
    within 1e-12 of the header's formula on the device's own sums (the variance relative to q / s + (mu' - mu)^2, the two numbers it is the
    difference of); R within 1e-12 of sum_k |p_k (u - mu_k) / var_k| and W of sum_k p_k / var_k, both exactly 0 off Omega.
    'floor': a class sits at the variance floor of 1e-6 inside the data, the exponent l_k reaches 1.8e5 and its rounding, eps |l_k|, goes
    into the posteriors: there the bound is 1e-12 (1 + max_k |l_k|), the maximum taken from the long-double run.
    'dying': the third class' posteriors underflow to exactly 0: s = 0, pi = 0, mu and var kept; a second step with that pi = 0 (lc = -inf
    on the device) stays finite and within the bar for the other classes."""
    d = bn.em_input(name)
    v, mask, y, idx = device_domain("em", name)
    amp = d["floor"]
    classes = tuple(np.asarray(a, dtype=np.float64) for a in d["classes"])
    got = bias.bias_em(y, d["b"], idx, np.concatenate(classes), n_em=1, want_rw=True)
    new = em_compare(name, 0, y, d["b"], idx, classes, got, amp)
    if name == "big":
        assert got["part"].shape[2] == 260
    if name == "floor":
        assert classes[1][2] == bn.VAR_FLOOR and bn.em_reference(y, d["b"], idx, *classes)["lmax"] > 1e3
    if name == "bfield":
        assert np.abs(d["b"]).max() > 0.05
        zero = bias.bias_em(y, np.zeros_like(d["b"]), idx, np.concatenate(classes), n_em=1)
        assert not np.array_equal(zero["sums"], got["sums"])
    if name == "dying":
        assert got["sums"][0][2] == 0.0 and np.all(got["part"][:, 2, :] == 0.0)
        assert new[2][2] == 0.0 and new[0][2] == 20.0 and new[1][2] == 1e-6
        again = bias.bias_em(y, d["b"], idx, new.reshape(-1), n_em=1, want_rw=True)
        after = em_compare(name, 1, y, d["b"], idx, tuple(new), again, amp)
        assert after[2][2] == 0.0 and after[0][2] == 20.0 and after[1][2] == 1e-6 and np.all(again["part"][:, 2, :] == 0.0)


def test_a_dead_class_stays_dead(bias):
    """bias_numpy.revive_input: the third class dies in the first of two steps of ONE call, so the second E-step runs with the log coefficient
    bias_mstep_kernel left for it.  Were that finite, the class would come back with a weight of 1e-133 at the voxel at 8 and take its mean
    from it (tests/test_bias_host.py shows both).  Also a dead class given as input (pi = 0) in the middle of the data takes nothing."""
    yv, classes = bn.revive_input()
    idx = np.arange(yv.size, dtype=np.int32)
    b = np.zeros(yv.shape)
    one = bias.bias_em(yv, b, idx, np.concatenate(classes), n_em=1)
    assert one["sums"][0][2] == 0.0 and np.all(one["part"][:, 2, :] == 0.0)
    two = bias.bias_em(yv, b, idx, np.concatenate(classes), n_em=2, want_rw=True)
    mu, var, pi = two["classes"].reshape(3, 3)
    assert np.all(two["part"][:, 2, :] == 0.0) and pi[2] == 0.0 and mu[2] == 9.5237 and var[2] == 1e-3
    assert np.isfinite(two["classes"]).all() and np.isfinite(two["rw"]).all() and abs(pi.sum() - 1.0) <= 1e-14
    # the fp64 restatement's two steps: the same classes within the bar (its sums differ from the device's only in their order)
    m, v, p = (a.copy() for a in classes)
    u = yv.reshape(-1)
    for _ in range(2):
        bn.m_step(bn.e_step(u, m, v, p), u, m, v, p)
    err = float(max(np.abs(mu / m - 1.0).max(), np.abs(var / v - 1.0).max(), np.abs(pi - p).max()))
    record("em revive", {"classes_rel": err})
    assert err <= BAR and p[2] == 0.0
    # pi = 0 as input, the class in the middle of the data: lc = -inf by the entry's rule
    mid = (np.array([6.3, 6.9, 6.6]), np.array([0.01, 0.01, 0.05]), np.array([0.5, 0.5, 0.0]))
    got = bias.bias_em(yv, b, idx, np.concatenate(mid), n_em=1, want_rw=True)
    pair = bias.bias_em(yv, b, idx, np.concatenate([a[:2] for a in mid]), n_em=1, want_rw=True)
    assert np.all(got["part"][:, 2, :] == 0.0) and np.array_equal(got["part"][:, :2, :], pair["part"]) and np.array_equal(got["rw"], pair["rw"])
    assert np.array_equal(got["classes"].reshape(3, 3)[:, :2], pair["classes"].reshape(3, 2)) and got["classes"][8] == 0.0


def test_em_steps_chain_and_faces(bias):
    """n_em steps in one call are n_em calls of one step, bit for bit; n_em = 0 gives R, W of the classes as they came; tensors in, tensors out"""
    d = bn.em_input("plain")
    v, mask, y, idx = device_domain("em", "plain")
    c = np.concatenate(d["classes"])
    three = bias.bias_em(y, d["b"], idx, c, n_em=3, want_rw=True)
    for _ in range(3):
        one = bias.bias_em(y, d["b"], idx, c, n_em=1, want_rw=True)
        c = one["classes"]
    for k in ("part", "sums", "classes", "rw"):
        assert np.array_equal(three[k], one[k]), k
    zero = bias.bias_em(y, d["b"], idx, c, n_em=0, want_rw=True)
    assert zero["part"] is None and np.array_equal(zero["classes"], c) and np.array_equal(zero["rw"], one["rw"])
    t = bias.bias_em(torch.as_tensor(y, device="cuda"), torch.as_tensor(d["b"], device="cuda"), torch.as_tensor(idx, device="cuda"),
                     np.concatenate(d["classes"]), n_em=3, want_rw=True)
    assert torch.is_tensor(t["rw"]) and t["rw"].is_cuda and np.array_equal(t["rw"].cpu().numpy(), three["rw"])
    assert np.array_equal(t["classes"], three["classes"]) and bias.bias_em(y, d["b"], idx, c, n_em=1)["rw"] is None


@pytest.mark.parametrize("name", bn.SMOOTH_INPUTS)
def test_smooth(bias, name):
    """Against the long-double smooth_axis, pointwise within 1e-12 of sum_t |w_t x_t| (of the three passes chained for 'all3' and 'flat':
    the passes' errors add up to a few fp64 roundings per tap, far inside the bar)"""
    a, radii, weights, axis = bn.smooth_input(name)
    got = bias.bias_smooth(a, radii, weights, axis)
    ref, mag = bn.smooth_reference(a, radii, weights, axis)
    assert got.shape == a.shape and np.isfinite(got).all()
    err = float((np.abs(got - ref) / mag).max())
    record("smooth " + name, {"shape": list(a.shape[:3]), "radii": list(radii), "axis": axis, "rel": err})
    assert err <= BAR
    if axis is None:                                                   # the three passes in one call are the three calls in turn, bit for bit
        step = a
        for ax in range(3):
            step = bias.bias_smooth(step, radii, weights, ax)
        assert np.array_equal(step, got)
        assert min(n for n, r in zip(a.shape, radii) if r) < max(radii)  # an axis shorter than its radius
    else:
        L, r = a.shape[axis], radii[axis]
        # one nonzero sample at the first and the last position of every tile, another place per channel: the reversed weights, placed exactly
        for i0 in sorted({0, 63, 64, 127, 128, L - 1} & set(range(L))):
            imp = np.zeros_like(a)
            at0, at1 = [0, 0, 0], [n - 1 for n in a.shape[:3]]
            at0[axis], at1[axis] = i0, L - 1 - i0
            imp[tuple(at0) + (0,)] = 1.0
            imp[tuple(at1) + (1,)] = 1.0
            out = bias.bias_smooth(imp, radii, weights, axis)
            want = np.zeros_like(a)
            for ch, at in ((0, at0), (1, at1)):
                for i in range(max(0, at[axis] - r), min(L, at[axis] + r + 1)):
                    to = list(at)
                    to[axis] = i
                    want[tuple(to) + (ch,)] = weights[axis][at[axis] - i + r]
            assert np.array_equal(out, want), (name, i0)


def test_smooth_radius_zero_aliasing_and_tensor_face(bias):
    a, radii, weights, axis = bn.smooth_input("A1_65")
    ident = [np.ones(1)] * 3
    for ax in (0, 1, 2, None):
        assert np.array_equal(bias.bias_smooth(a, (0, 0, 0), ident, ax), a)
    t = torch.as_tensor(a, device="cuda")
    got = bias.bias_smooth(t, radii, weights, axis)
    assert torch.is_tensor(got) and np.array_equal(got.cpu().numpy(), bias.bias_smooth(a, radii, weights, axis))
    assert np.array_equal(t.cpu().numpy(), a)                          # the input is left alone
    lib = importlib.import_module(PKG + "._lib")
    with pytest.raises(lib.Met2Error):
        bias.bias_smooth(a, (65, 0, 0), [np.ones(131) / 131.0, np.ones(1), np.ones(1)], 0)


@pytest.mark.parametrize("name", bn.UPDATE_INPUTS)
def test_update(bias, name):
    """b moves only where S_W > 0 and is bit-equal to its input elsewhere; the mean over the list within 1e-12 of the mean of |b| + |S_R / S_W|;
    the new b within 1e-12 of |b| + |S_R / S_W| + |mean|.  The list is a part of the support D, so recentring over the list's voxels alone,
    or over more than D, shows."""
    b, S, idx = bn.update_input(name)
    nb, bmean = bias.bias_update(b, S, idx)
    ref, bml, scale = bn.update_reference(b, S, idx)
    D = S[..., 1] > 0
    assert np.array_equal(nb[~D], b[~D]) and np.all(nb[D] != b[D]) and np.isfinite(nb).all()
    e_mean = float(abs(bmean - bml) / (np.abs(b).mean() + np.abs(S[..., 0][D] / S[..., 1][D]).mean()))
    e_b = float((np.abs(nb - ref)[D] / scale[D]).max())
    record("update " + name, {"n": int(b.size), "N": int(idx.size), "bmean_rel": e_mean, "b_rel": e_b})
    assert e_mean <= BAR and e_b <= BAR
    assert abs(float(nb.reshape(-1)[idx].astype(LD).mean())) <= BAR * float(np.abs(nb).mean())      # centred on the list
    if name == "big":
        assert -(-idx.size // 1024) > 256
    if name == "small":
        same, m0 = bias.bias_update(b, S, idx[:0])                      # an empty list: b moves, nothing is recentred
        moved = b.copy()
        moved[D] += S[..., 0][D] / S[..., 1][D]
        assert m0 == 0.0 and np.array_equal(same, moved)
        t, mt = bias.bias_update(torch.as_tensor(b, device="cuda"), torch.as_tensor(S, device="cuda"), torch.as_tensor(idx, device="cuda"))
        assert torch.is_tensor(t) and mt == bmean and np.array_equal(t.cpu().numpy(), nb)


def chain(bias, v, mask, vox, n_class=3, n_outer=4, n_em=10, fwhm=20.0):
    """met2_bias_field restated with the stage entries, every array passing through the host between two of them"""
    y, idx = bias.bias_domain(v, mask)
    ini = bias.bias_init(y, idx, n_class)
    classes = ini["classes"]
    b = np.zeros(v.shape)
    radii, weights = bias.bias_weights(vox, fwhm)
    if not ini["degenerate"]:
        for _ in range(n_outer):
            em = bias.bias_em(y, b, idx, classes, n_em=n_em, want_rw=True)
            classes = em["classes"]
            b, _ = bias.bias_update(b, bias.bias_smooth(em["rw"], radii, weights), idx)
    out, field = bias.bias_apply(v, b)
    return out, field, classes


@pytest.mark.parametrize("name", ("phantom", "holes", "k8floor", "seams"))
def test_the_stages_chained_are_the_filter(bias, name):
    """out, field and classes bit-equal to met2_bias_field: the entries run the filter's own host code and kernels"""
    motor = importlib.import_module(PKG + ".motor")
    v, mask, vox, kw = bn.case(name)
    want = motor.bias_field_filter(v, mask, vox, return_field=True, **kw)
    got = chain(bias, v, mask, vox, **kw)
    for g, w, what in zip(got, want, ("out", "field", "classes")):
        assert np.array_equal(g, w, equal_nan=True), (name, what, float(np.nanmax(np.abs(g - w))))


def test_weights_are_the_restatement_s(bias):
    """the host's radii and weights against the long-double restatement: 1e-15 absolute on weights that sum to 1"""
    worst = 0.0
    for vox in [bn.case(name)[2] for name in bn.CASES] + [(0.53, 1.0, 80.0)]:
        radii, weights = bias.bias_weights(vox)
        for a in range(3):
            r, w = bn.radius_weights(20.0, vox[a], LD)
            assert radii[a] == r and weights[a].shape == (2 * r + 1,)
            worst = max(worst, float(np.abs(weights[a] - w).max()))
    record("weights", {"abs": worst})
    assert worst <= 1e-15
    lib = importlib.import_module(PKG + "._lib")
    with pytest.raises(lib.Met2Error):
        bias.bias_weights((0.5, 2.0, 2.0))                               # r = 68


def test_stage_return_codes(bias):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    import ctypes as C
    y = torch.zeros(8, dtype=torch.float64, device="cuda")
    idx = torch.arange(8, dtype=torch.int32, device="cuda")
    cls = (C.c_double * 3)(0.0, 1.0, 1.0)
    N = C.c_int64(5)
    assert L.met2_bias_domain(0, -1, 2, 2, y.data_ptr(), None, y.data_ptr(), idx.data_ptr(), C.byref(N), None) == -1
    assert L.met2_bias_domain(0, 0, 2, 2, None, None, None, None, C.byref(N), None) == 0 and N.value == 0
    assert L.met2_bias_domain(0, 2, 2, 2, None, None, y.data_ptr(), idx.data_ptr(), C.byref(N), None) == -1
    assert L.met2_bias_init(0, 8, y.data_ptr(), idx.data_ptr(), 9, 3, None, None, None, None, None) == -1
    assert L.met2_bias_init(0, 8, y.data_ptr(), idx.data_ptr(), 8, 0, None, None, None, None, None) == -1
    assert L.met2_bias_init(0, 8, y.data_ptr(), idx.data_ptr(), 8, 9, None, None, None, None, None) == -2
    assert L.met2_bias_init(0, 0, y.data_ptr(), idx.data_ptr(), 0, 3, None, None, None, None, None) == -1
    em = lambda c, n_em=1, N=8, K=1: L.met2_bias_em(0, 8, y.data_ptr(), y.data_ptr(), idx.data_ptr(), N, K, c, n_em, None, None, None, None)
    assert em(cls) == 0 and em(cls, n_em=-1) == -1 and em(cls, N=0) == -1 and em(None) == -1 and em(cls, K=9) == -2 and em(cls, K=0) == -1
    for bad in ((float("nan"), 1.0, 1.0), (0.0, 0.0, 1.0), (0.0, -1.0, 1.0), (0.0, float("inf"), 1.0), (0.0, 1.0, -0.5), (0.0, 1.0, float("nan"))):
        assert em((C.c_double * 3)(*bad)) == -1
    r = (C.c_int32 * 3)(1, 1, 1)
    w = (C.c_double * 9)(*([1.0 / 3.0] * 9))
    a = torch.zeros(16, dtype=torch.float64, device="cuda")
    sm = lambda r=r, axis=-1, nx=2: L.met2_bias_smooth(0, nx, 2, 2, a.data_ptr(), r, w, axis, a.data_ptr(), None)
    assert sm() == 0 and sm(axis=3) == -1 and sm(axis=-2) == -1 and sm(nx=-1) == -1 and sm(nx=0) == 0
    assert sm(r=(C.c_int32 * 3)(1, -1, 1)) == -1 and sm(r=(C.c_int32 * 3)(1, 65, 1)) == -2
    assert L.met2_bias_update(0, 8, y.data_ptr(), a.data_ptr(), idx.data_ptr(), 9, None, None) == -1
    assert L.met2_bias_update(0, 8, None, a.data_ptr(), idx.data_ptr(), 8, None, None) == -1
    assert L.met2_bias_apply(0, 8, y.data_ptr(), y.data_ptr(), y.data_ptr(), None, None) == -1      # in place
    assert L.met2_bias_apply(0, 0, None, None, None, None, None) == 0 and L.met2_bias_apply(0, -1, None, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert bool((y == 0.0).all()) and bool((a == 0.0).all())
    with pytest.raises(ValueError):
        bias.bias_init(np.zeros((2, 2, 2)), np.array([8], dtype=np.int32))       # an index outside the volume is refused before the call
    with pytest.raises(ValueError):
        bias.bias_em(np.zeros((2, 2, 2)), np.zeros((2, 2, 2)), np.array([-1], dtype=np.int32), [0.0, 1.0, 1.0])
