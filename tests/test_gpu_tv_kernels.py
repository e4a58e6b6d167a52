"""GPU tests of the TV denoiser's kernels one by one (csrc/met2_tv.hip through met2_tv_detail, met2_tv_sigma and met2_tv_chambolle -- the
three entries launch the detail and sigma kernels through the same host helpers).
  detail   every coefficient against oracle/tv_oracle.py (itself pinned to a second transcription in tests/test_tv_host.py), bit for
           bit: same products, same sums, same order, contraction off.
  sigma    against np.median on coefficients built to reach each path of the bisection -- the counting passes, the LDS list, the
           fall-back on the array when more than the cap of keys are equal, and both answers for the upper middle value of an even
           count.  Each case first asserts, with a restatement of the bisection's bookkeeping (`trace`), that its input takes that path.
  iterate  the whole denoiser on volumes whose sizes sit on the tile seams (asserted with tv_launch_info), two echoes that stop at
           different iterations, inputs whose stopping decision is not within rounding of the threshold (asserted on the energies).
Nothing here hard-codes the tile geometry or the cap: they come from tv_launch_info."""
import importlib

import numpy as np
import pytest
import torch

from oracle import tv_oracle
from test_tv import _check, _phantom, _want
from test_tv_host import DETAIL_SHAPES

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
PHI = 0.6744897501960817
DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def tv():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".tv")


@pytest.fixture(scope="module")
def cap(tv):
    return tv.tv_launch_info(8, 8, 8)["sigma_cap"]


def _fortran(vol):
    """[nx,ny,nz,nt] as the Fortran-ordered device tensor nibabel's arrays become: echo-major in memory"""
    t = torch.as_tensor(np.asfortranarray(vol), device=torch.device("cuda", 0))
    assert t.permute(3, 2, 1, 0).is_contiguous()
    return t


# ---- C1: tv_detail_kernel, per element -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["C", "F"])
def test_detail_kernel_matches_the_restatement_bit_for_bit(tv, layout):
    rng = np.random.default_rng(23)
    for shape in DETAIL_SHAPES:
        vol = rng.standard_normal(shape + (3,)) * 10.0 ** rng.integers(-2, 3, shape + (3,))
        want = np.stack([tv_oracle.detail_coefficients(vol[..., t]) for t in range(3)], axis=3)
        if layout == "C":
            got = tv.tv_detail_coefficients(vol)
        else:
            got = tv.tv_detail_coefficients(_fortran(vol)).cpu().numpy()
        assert got.shape == want.shape, shape
        err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(vol)))
        assert np.array_equal(got, want), (shape, err)


# ---- C2: tv_sigma_kernel on supplied coefficients ------------------------------------------------------------------------------------
def trace(d, cap):
    """The bookkeeping of tv_sigma_kernel's bisection for one echo, restated on sorted keys: which path decides the last bits, at which
    bit the two-bit passes stopped, and which of the two answers an even count takes."""
    d = np.asarray(d, dtype=np.float64)
    keys = np.sort(np.abs(d[d != 0]).view(np.uint64))
    m = int(keys.size)
    if m == 0:
        return {"m": 0}
    below_of = lambda c: int(np.searchsorted(keys, np.uint64(c), side="left"))
    k1 = (m - 1) // 2
    prefix, below, inb, bit, shared = 0, 0, m, 62, []
    while inb > cap and bit >= 1:
        q = 1 << (bit - 1)
        r = [below_of(prefix + j * q) for j in (1, 2, 3)]
        e = below + inb
        if r[2] <= k1:
            prefix, below, inb = prefix + 3 * q, r[2], e - r[2]
        elif r[1] <= k1:
            prefix, below, inb = prefix + 2 * q, r[1], r[2] - r[1]
        elif r[0] <= k1:
            prefix, below, inb = prefix + q, r[0], r[1] - r[0]
        else:
            inb = r[0] - below
        bit -= 2
        shared.append(inb)
    a = keys[k1]
    nle = int(np.searchsorted(keys, a, side="right"))
    return {"m": m, "k1": k1, "path": "list" if inb <= cap else "array", "bit": bit, "passes": len(shared), "shared": shared,
            "a": float(a.view(np.float64)), "repeated": nle >= k1 + 2, "run": nle - below_of(a), "run_end": nle - 1}


def sigma_ref(d):
    d = np.asarray(d, dtype=np.float64).ravel()
    d = d[d != 0]
    if d.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        return float(np.median(np.abs(d)) / PHI) if np.isfinite(d).all() else float("nan")


def copy_ref(w):
    return (~((w > 0.0) & (w <= DBL_MAX))).astype(np.int32)


def check_sigma(tv, coef, factor=2.0, weight=None):
    coef = np.atleast_2d(np.asarray(coef, dtype=np.float64))
    sig, w, cp = tv.tv_sigma_from_coefficients(coef, weight=weight, weight_factor=factor)
    want = np.array([sigma_ref(c) for c in coef])
    assert np.array_equal(sig, want, equal_nan=True), (sig, want)
    with np.errstate(invalid="ignore", over="ignore"):
        ww = factor * want if weight is None else np.broadcast_to(np.asarray(weight, dtype=np.float64), want.shape)
        assert np.array_equal(w, ww, equal_nan=True), (w, ww)
        assert np.array_equal(cp, copy_ref(ww)), (cp, ww)
    return sig, w, cp


def _scatter(values, nc, rng):
    """`values` at random places among zeros"""
    out = np.zeros(nc)
    out[rng.permutation(nc)[:len(values)]] = values
    return out


NC = 20000


def test_sigma_counts_from_one_value_to_past_the_cap(tv, cap):
    """The masked-volume pattern: m non-zero coefficients among zeros.  Up to the cap the list is filled at once (no counting pass), one
    past it the counting passes run first."""
    rng = np.random.default_rng(31)
    assert NC > 2 * cap + 1
    for m in (1, 2, 3, 4, cap - 1, cap, cap + 1, 2 * cap + 1):
        c = _scatter(rng.standard_normal(m) * 3.0, NC, rng)
        tr = trace(c, cap)
        assert tr["m"] == m and tr["path"] == "list" and (tr["passes"] == 0) == (m <= cap) and (m <= cap or tr["bit"] >= 1), (m, tr)
        check_sigma(tv, c)
    # the same few values when nothing is zero, and when the array is shorter than a wave
    for m in (1, 2, 3, 4, 63, 65):
        check_sigma(tv, rng.standard_normal(m))


@pytest.mark.parametrize("family", ["normal", "300 decades"])
def test_sigma_continuous_values_reach_the_list_after_counting_passes(tv, cap, family):
    rng = np.random.default_rng(37)
    for n in (NC, NC - 1):                                                          # an even and an odd count
        c = rng.standard_normal(n) if family == "normal" else rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-150.0, 150.0, n)
        tr = trace(c, cap)
        assert tr["m"] == n > cap and tr["path"] == "list" and tr["passes"] >= 1 and tr["bit"] >= 1 and not tr["repeated"], tr
        check_sigma(tv, c)


def _equal_run(lower, run, upper, rng, value=1.5):
    """`lower` distinct values under `value`, `run` copies of it, `upper` distinct values above, shuffled, signs mixed, among zeros"""
    v = np.concatenate([rng.uniform(0.1, 0.9 * value, lower), np.full(run, value), rng.uniform(1.1 * value, 9.0, upper)])
    assert np.unique(v).size == lower + upper + 1
    return _scatter(v * rng.choice([-1.0, 1.0], v.size), NC, rng)


def test_sigma_more_than_the_cap_of_equal_keys_at_the_median(tv, cap):
    """The fall-back: the counting passes run out of bits with more than the cap of keys left, bit 0 is decided on the array."""
    rng = np.random.default_rng(41)
    run = cap + 500
    cases = {"odd count": (300, run, 401), "even count, the run covers both middle positions": (300, run, 400),
             "even count, the run ends at the lower middle": (100, run, 100 + run),
             "even count, the run starts at the upper middle": (100 + run, run, 100),
             "even count, nothing but the run": (0, run + 1, 0), "odd count, nothing but the run": (0, run, 0)}
    for name, (lo, n, hi) in cases.items():
        c = _equal_run(lo, n, hi, rng)
        tr = trace(c, cap)
        assert tr["m"] == lo + n + hi <= NC, name
        if "starts at the upper" in name:                                           # the lower middle is the last value under the run: list path
            assert tr["a"] < 1.5 and not tr["repeated"] and tr["path"] == "list", (name, tr)
        else:
            assert tr["path"] == "array" and tr["bit"] == 0 and tr["a"] == 1.5 and tr["run"] == n > cap, (name, tr)
        if "covers both" in name or "nothing but" in name:
            assert tr["repeated"] or tr["m"] % 2 == 1, (name, tr)
        if "ends at the lower" in name:
            assert tr["m"] % 2 == 0 and tr["run_end"] == tr["k1"] and not tr["repeated"], (name, tr)
        check_sigma(tv, c)


def test_sigma_keys_that_differ_in_the_last_two_bits_around_the_median(tv, cap):
    """Four neighbouring doubles (np.nextafter), so the median is decided by bit 1 and bit 0.  With more than the cap of keys in a pair
    that shares all but bit 0, that bit is decided on the array between two DIFFERENT keys; with few of them, on the list.  The lower
    middle position is put inside a key's run and on the last copy of keys 0, 1 and 2, where the upper middle value is the next key."""
    rng = np.random.default_rng(43)
    v = [1.5]
    for _ in range(3):
        v.append(float(np.nextafter(v[-1], 4.0)))
    assert [int(np.float64(x).view(np.uint64)) & 3 for x in v] == [0, 1, 2, 3]
    for unit, want_path in ((cap // 12, "array"), (3, "list")):
        n = [7 * unit, 6 * unit, 8 * unit, 7 * unit]
        assert (min(n[0] + n[1], n[2] + n[3]) > cap) == (want_path == "array")
        ends = np.cumsum(n) - 1                                                     # the last copy of each key, within the block of four
        places = [(n[0] + n[1] // 2, 0, 1), (n[0] + n[1] // 2, 1, 1), (ends[0], 0, 0), (ends[1], 0, 1), (ends[2], 0, 2), (ends[2] + n[3] // 2, 1, 3),
                  (ends[0], 1, 0), (ends[2] + 1, 0, 3)]
        for off, odd, key in places:                                                # lower middle at block position `off`, in key `key`
            lower = max(10, sum(n) - 2 * off) + 10 + (cap if want_path == "list" else 0)     # few neighbours among many other values
            upper = lower + 2 * off + (1 if odd else 2) - sum(n)
            vals = np.concatenate([rng.uniform(0.1, 1.0, lower)] + [np.full(k, x) for k, x in zip(n, v)] + [rng.uniform(2.0, 3.0, upper)])
            c = _scatter(vals * rng.choice([-1.0, 1.0], vals.size), vals.size + 1000, rng)
            tr = trace(c, cap)
            assert tr["m"] % 2 == odd and tr["k1"] == lower + off and tr["a"] == v[key], (unit, off, odd, tr)
            assert tr["path"] == want_path and tr["passes"] >= 1, (unit, off, odd, tr)
            assert want_path == "list" or (tr["bit"] == 0 and tr["shared"][-1] > cap), (unit, off, odd, tr)
            if not odd:
                assert tr["repeated"] == (off not in ends), (unit, off, tr)
            check_sigma(tv, c)


def test_sigma_signs_zeros_and_denormals(tv, cap):
    rng = np.random.default_rng(47)
    tiny = np.float64(5e-324)
    fam = {
        "all negative": -np.abs(rng.standard_normal(NC)) - 0.1,
        "-0.0 counts as zero": np.where(rng.random(NC) < 0.5, -0.0, rng.standard_normal(NC)),
        "only -0.0 and +0.0": np.where(rng.random(NC) < 0.5, -0.0, 0.0),
        "denormals": rng.integers(-2000, 2001, NC) * tiny,
        "few denormals among zeros": _scatter(rng.integers(1, 100, 101) * tiny * rng.choice([-1.0, 1.0], 101), NC, rng),
        "denormals and normals": np.where(rng.random(NC) < 0.5, rng.integers(1, 1 << 40, NC) * tiny, rng.standard_normal(NC) * 1e-300),
        "the largest finite values": rng.choice([-1.0, 1.0], NC) * DBL_MAX * rng.uniform(0.3, 0.45, NC),
    }
    assert np.signbit(fam["-0.0 counts as zero"][fam["-0.0 counts as zero"] == 0]).any()
    for name, c in fam.items():
        tr = trace(c, cap)
        sig, w, cp = check_sigma(tv, c)
        if name == "only -0.0 and +0.0":
            assert tr["m"] == 0 and sig[0] == 0.0 and cp[0] == 1
        else:
            assert tr["m"] > 0 and sig[0] > 0.0, name
    sig, w, cp = check_sigma(tv, fam["the largest finite values"], factor=4.0)       # weight = factor x sigma overflows: copied through
    assert np.isinf(w[0]) and cp[0] == 1


def test_sigma_non_finite_all_zero_and_explicit_weights(tv, cap):
    rng = np.random.default_rng(53)
    base = rng.standard_normal(NC)
    for bad, at in ((np.inf, 0), (-np.inf, NC - 1), (np.nan, NC // 2), (np.nan, 1023), (np.inf, 1024)):
        c = base.copy(); c[at] = bad
        sig, w, cp = check_sigma(tv, c)
        assert np.isnan(sig[0]) and np.isnan(w[0]) and cp[0] == 1
    sig, w, cp = check_sigma(tv, np.zeros(NC))
    assert sig[0] == 0.0 and w[0] == 0.0 and cp[0] == 1
    sig, w, cp = check_sigma(tv, np.zeros(1))
    assert sig[0] == 0.0 and cp[0] == 1
    # explicit weights: reported as given, sigma still estimated, copy from the weight alone
    coef = np.stack([base, np.zeros(NC), base * 2.0, base, base, base])
    wts = np.array([3.0, 1.0, 0.0, -1.0, np.inf, np.nan])
    sig, w, cp = check_sigma(tv, coef, weight=wts)
    assert list(cp) == [0, 0, 1, 1, 1, 1] and sig[1] == 0.0 and sig[2] == 2.0 * sig[0]
    assert [int(x) for x in check_sigma(tv, coef[:2], factor=0.0)[2]] == [1, 1]      # weight_factor = 0: every echo copied through


def test_sigma_echoes_of_different_families_in_one_launch_and_determinism(tv, cap):
    """Five echoes that take different paths in ONE launch give the bits of five launches of one echo; the same input twice gives the
    same bits (the LDS list is filled with atomics in arbitrary order: the count under a threshold does not depend on it)."""
    rng = np.random.default_rng(59)
    coef = np.stack([rng.standard_normal(NC), _scatter(rng.standard_normal(5), NC, rng), _equal_run(300, cap + 500, 400, rng), np.zeros(NC),
                     _equal_run(100, cap + 500, cap + 600, rng)])
    paths = [trace(c, cap).get("path") for c in coef]
    assert paths == ["list", "list", "array", None, "array"]
    bad = coef.copy(); bad[1, 7] = np.nan
    for arr in (coef, bad):
        together = check_sigma(tv, arr)
        alone = [tv.tv_sigma_from_coefficients(c) for c in arr]
        for k in range(3):
            assert np.array_equal(together[k], np.concatenate([a[k] for a in alone]), equal_nan=True)
        again = tv.tv_sigma_from_coefficients(arr)
        for k in range(3):
            assert np.array_equal(together[k], again[k], equal_nan=True)


def test_sigma_ties_end_to_end_on_a_period_two_volume(tv, cap):
    """A volume of period 2 along every axis: most interior coefficients are bit-equal, more of them than the cap.  The detail kernel, the
    sigma kernel's fall-back and the denoiser's sigma all give the restatement's bits."""
    a, b, c = np.array([1.0, 4.0]), np.array([2.0, 7.0]), np.array([3.0, 5.0])
    i = np.arange(40) % 2
    vol = a[i][:, None, None] * b[i][None, :, None] * c[i][None, None, :] + 10.0
    d = tv_oracle.detail_coefficients(vol)
    assert d.size == tv.tv_launch_info(40, 40, 40)["nc"]
    _, counts = np.unique(np.abs(d[d != 0]), return_counts=True)
    assert counts.max() > cap                                                       # the tie premise
    tr = trace(d.ravel(), cap)
    assert tr["path"] == "array" and tr["run"] == counts.max(), tr
    want = tv_oracle.estimate_sigma(vol)
    for data in (vol[..., None], _fortran(vol[..., None])):
        got = tv.tv_detail_coefficients(data)
        got = got.cpu().numpy() if torch.is_tensor(got) else got
        assert np.array_equal(got[..., 0], d)
        out, sig, its = tv.tv_chambolle(data, return_info=True)
        assert sig[0] == want and its[0] > 1, (sig, want, its)
    check_sigma(tv, d.ravel())


# ---- C3: the whole denoiser at the tile seams ----------------------------------------------------------------------------------------
def _last(n, step):
    return n - (-(-n // step) - 1) * step                                           # what the last tile / segment of an axis holds


# (n0, n1, n2) in memory order -> what the case is there for, as a predicate on the triple and its tv_launch_info
SEAMS = {
    (17, 15, 65): lambda n, g: g["nseg"] == 2 and _last(n[0], g["xlen"]) == 1 and g["step1"] == g["oy"] - 1 and _last(n[1], g["step1"]) == 1
                               and g["nt2"] == 2 and _last(n[2], g["step2"]) == 1,          # a segment of one plane, a tile of one row, a tile of one lane
    (16, 8, 64): lambda n, g: g["nseg"] == 1 and n[0] == g["xlen"] and n[1] == g["oy"] == g["step1"] and g["nt1"] == 1
                              and g["nt2"] == 1 and n[2] == g["step2"],                      # exactly one full tile: no halo row, no neighbour
    (33, 9, 129): lambda n, g: g["nseg"] == 3 and _last(n[0], g["xlen"]) == 1 and g["nt1"] == 2 and _last(n[1], g["step1"]) == 2
                               and g["nt2"] == 3 and _last(n[2], g["step2"]) == 1,          # the middle tile along n2 has neighbours on both sides
    (2, 16, 128): lambda n, g: g["nseg"] == 1 and g["xlen"] == n[0] and g["nt1"] == 3 and _last(n[1], g["step1"]) == 2
                               and g["nt2"] == 2 and _last(n[2], g["step2"]) == g["step2"],  # two full tiles along n2: the last one has no neighbour
    (17, 16, 63): lambda n, g: g["nseg"] == 2 and _last(n[0], g["xlen"]) == 1 and g["nt1"] == 3 and g["nt2"] == 1 and n[2] == g["step2"] - 1,
}
SEAM_SEED = 1          # found on the CPU: at every shape below the restatement's own stopping decision has the margin stable_stop asks for


def step_volume(shape, seed, noise=(2.0, 8.0)):
    """A 100-level step across an oblique plane (it crosses every tile seam), one echo per noise level"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    x, y, z = np.meshgrid(np.arange(nx) / nx, np.arange(ny) / ny, np.arange(nz) / nz, indexing="ij")
    base = 100.0 * ((x + 0.7 * y + 0.5 * z) > 1.0)
    return np.stack([base + s * rng.standard_normal(shape) for s in noise], axis=3)


def stable_stop(vol, eps=2.0e-4, max_num_iter=200):
    """The iteration count is compared exactly while the GPU adds the energy in another order than numpy.  A reordered sum moves E by
    about 1e-13 relative, E_prev - E is of order eps E, so the decision moves by about 5e-10 of the threshold eps E_init: the input must
    leave 1e-6 of the threshold on either side -- under it at the stopping iteration, over it at every iteration before."""
    ok = True
    for t in range(vol.shape[3]):
        v = np.ascontiguousarray(vol[..., t])
        _, n, E = tv_oracle.denoise_tv_chambolle(v, 2.0 * tv_oracle.estimate_sigma(v), eps, max_num_iter, return_iters=True, return_energies=True)
        thr = eps * E[0]
        if n < max_num_iter:
            ok = ok and n >= 2 and thr - abs(E[n - 2] - E[n - 1]) > 1e-6 * thr
        ok = ok and all(abs(E[i - 1] - E[i]) - thr > 1e-6 * thr for i in range(1, n - 1 if n < max_num_iter else n))
    return ok


@pytest.mark.parametrize("flip", [False, True], ids=["C has the triple", "F has the triple"])
@pytest.mark.parametrize("triple", list(SEAMS))
def test_denoiser_at_the_tile_seams_in_both_layouts(tv, triple, flip):
    """[nx,ny,nz] = the triple: the C-ordered run meets the seams as listed; reversed: the Fortran-ordered run does (nx is then the
    contiguous axis).  Both layouts run on both, so every seam is met as n0 and as n2 by both instances of the kernel."""
    shape = triple[::-1] if flip else triple
    g = tv.tv_launch_info(*shape, 2, 1 if flip else 0)
    assert SEAMS[triple](triple, g), (triple, g)
    vol = step_volume(shape, SEAM_SEED)
    assert stable_stop(vol)                                                         # a condition on the input, before the GPU is looked at
    want = _want(vol)
    assert want[2][0] != want[2][1], want[2]                                        # the echoes stop at different iterations
    got, sig, its = tv.tv_chambolle(vol, return_info=True)
    _check(vol, got, sig, its, want=want)
    gf, sf, itf = tv.tv_chambolle(_fortran(vol), return_info=True)
    _check(vol, gf.cpu().numpy(), sf, itf, want=want)
    assert np.array_equal(sf, sig)


@pytest.mark.parametrize("layout", ["C", "F"])
def test_result_parity_after_one_two_and_three_iterations(tv, layout):
    """The result is taken from the buffer the last executed iteration read (`parity`); one iteration returns the input itself."""
    shape = (17, 15, 65)
    vol = step_volume(shape, 3)
    data = vol if layout == "C" else _fortran(vol)
    for k in (1, 2, 3):
        got, sig, its = tv.tv_chambolle(data, max_num_iter=k, return_info=True)
        got = got.cpu().numpy() if torch.is_tensor(got) else got
        assert list(its) == [k, k]
        for t in range(2):
            v = np.ascontiguousarray(vol[..., t])
            want = tv_oracle.denoise_tv_chambolle(v, 2.0 * tv_oracle.estimate_sigma(v), max_num_iter=k)
            assert np.max(np.abs(got[..., t] - want)) <= 1e-12 * np.max(np.abs(want)), (k, t)
            if k == 1:
                assert np.array_equal(got[..., t], v)
            else:
                assert not np.array_equal(got[..., t], v)


def test_echo_count_at_the_gather_kernels_lds_limit(tv):
    """C order goes through the gather's LDS tile of 64 x (nt + 1) doubles: 127 echoes are exactly 64 KiB, 128 are refused; a
    Fortran-ordered volume is echo-major already and takes any count."""
    L = importlib.import_module(PKG + "._lib")
    assert 8 * 64 * (127 + 1) == 65536
    vol = _phantom((3, 3, 5), 128, seed=61)
    assert stable_stop(vol)
    got, sig, its = tv.tv_chambolle(vol[..., :127], return_info=True)
    want = _want(vol)
    _check(vol[..., :127], got, sig, its, want=(want[0][..., :127], want[1][:127], want[2][:127]))
    with pytest.raises(L.Met2Error):
        tv.tv_chambolle(torch.as_tensor(vol, device=torch.device("cuda", 0)))
    with pytest.raises(L.Met2Error):
        tv.tv_detail_coefficients(vol)
    gf, sf, itf = tv.tv_chambolle(_fortran(vol), return_info=True)
    _check(vol, gf.cpu().numpy(), sf, itf, want=want)
    assert len(set(itf.tolist())) > 1
    d = tv.tv_detail_coefficients(_fortran(vol)).cpu().numpy()
    assert np.array_equal(d[..., 127], tv_oracle.detail_coefficients(vol[..., 127]))
    assert np.array_equal(tv.tv_detail_coefficients(vol[..., :127])[..., 126], tv_oracle.detail_coefficients(vol[..., 126]))


def test_polling_interval_never_changes_the_result(tv):
    vol = step_volume((17, 15, 65), 3)
    ref = tv.tv_chambolle(vol, return_info=True)
    assert ref[2][0] != ref[2][1] and (ref[2] > 1).all()
    for poll in (1000, 1, 0):                                                       # never polls; polls after every iteration; enqueues all
        got = tv.tv_chambolle(vol, poll_every=poll, return_info=True)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), poll


def test_fortran_ordered_volume_denoised_in_place(tv):
    L = importlib.import_module(PKG + "._lib")
    shape, nt = (65, 15, 17), 2
    vol = step_volume(shape, 3)
    tf = _fortran(vol)
    want, sig, its = tv.tv_chambolle(tf, return_info=True)
    td = tf.clone(memory_format=torch.preserve_format)
    assert td.stride() == tf.stride() and td.data_ptr() != tf.data_ptr()
    dev = td.device
    nb = int(L.lib().met2_tv_work_bytes(*shape, nt, 1))
    work = torch.empty(nb, dtype=torch.uint8, device=dev)
    s2 = torch.empty(nt, dtype=torch.float64, device=dev); i2 = torch.empty(nt, dtype=torch.int32, device=dev)
    L.check(L.lib().met2_tv_chambolle(0, *shape, nt, td.data_ptr(), 1, None, 2.0, 2e-4, 200, 4, td.data_ptr(), s2.data_ptr(), i2.data_ptr(), work.data_ptr(), nb,
                                      torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(td, want) and not torch.equal(td, tf)
    assert np.array_equal(s2.cpu().numpy(), sig) and np.array_equal(i2.cpu().numpy(), its)
