"""A voxel's fit must not depend on the rest of its launch (include/met2_hip.h, met2_fit_host: "bit for bit those of one met2_fit over the
whole list, whatever n_plans, chunk and the devices"; the chunked callers -- met2_fit_host, the bootstrap, the Monte-Carlo study -- rely on it).

The spill-over kernel (fit_kernel.hpp, fit_kernel<..., SECOND = true>) is where a voxel's path depends on the launch: it carves the workgroup's LDS
by the length of its queue -- w2 waves of capacity k2, the first kernel's capacity for a long queue, all of nT2 for a short one -- and the L-curve's
queued voxels go on from a saved sweep state only while records last (lc_cap).  Every test here fits the same voxels under two launch compositions
that take different branches there, asserts from the library's own counters that they did (the premises), and asserts bit-equality; the queued
voxels themselves are checked against the oracle at both capacities.  The carving is restated from the code (_carve), with the grid the plan
reports, not a CU count written down here."""
import importlib
import os

import numpy as np
import pytest

from conftest import relmax_rows

PKG = "multicomponent-t2-toolbox_amd"
pytestmark = pytest.mark.gpu
TOL = 1e-5
FIELDS = ("fsol", "sig", "reg", "lam", "maps", "status")
NTHREADS = min(16, os.cpu_count() or 1)
# (x2_lo, x2_hi, gcv_lo, gcv_hi, bayes_lo, bayes_hi): test_round5.py's non-default lambda-search intervals
INTERVALS = (0.05, 30.0, 1e-6, 4.0, 1e-6, 3.5)
IV_NAMES = ("x2_lo", "x2_hi", "gcv_lo", "gcv_hi", "bayes_lo", "bayes_hi")


def binom99(p, n):
    """one-sided 99 % upper limit of a count with rate p in n trials (test_tail_parity.py), at least 1: one Brent tie is always allowed"""
    return max(1, int(np.ceil(n * (p + 2.33 * np.sqrt(p * (1.0 - p) / n)))))


def _col_base(k):
    return k * (k + 1) // 2


def _carve(plan, method, nvox, ntail):
    """The spill-over kernel's LDS carving for a launch of nvox voxels with ntail of them queued, restated from fit_geometry (met2_hip.hip: the
    waves of a short list) and fit_kernel<SECOND = true> (fit_kernel.hpp: w2 waves of capacity k2)."""
    info = plan.launch_info(method)
    grid, wmax = info["grid"], info["block"] // 64
    wave_doubles = (info["lds_bytes"] - 64) // 8 // wmax
    per_cu = -(-nvox // grid)
    waves = min(wmax, max(4, -(-per_cu // 4) * 4))
    w2 = waves
    while w2 > 1 and (w2 - 1) * grid >= ntail:
        w2 -= 1
    per = (waves * wave_doubles // w2) & ~1
    k2 = 0
    while k2 < plan.n_t2 and _col_base(k2 + 1) <= per:
        k2 += 1
    return dict(grid=grid, waves=waves, w2=w2, k2=k2, ntail=ntail)


def _long_premise(plan, method, nvox, ntail, legs=True):
    c = _carve(plan, method, nvox, ntail)
    assert c["w2"] == c["waves"] and ntail > (c["waves"] - 1) * c["grid"], c       # every wave of the first kernel's layout runs queued voxels
    if legs:
        assert c["k2"] < plan.n_t2, c                                                  # ... at a capacity below nT2: the spill-over legs run
    else:
        assert c["k2"] == plan.n_t2, c                                                 # (a plan whose capacity is nT2 already: BayesReg, nT2 <= 64)
    return c


def _short_premise(plan, method, nvox, ntail):
    c = _carve(plan, method, nvox, ntail)
    assert 0 < ntail <= c["grid"] and c["w2"] == 1 and c["k2"] == plan.n_t2, c        # one wave per workgroup at full capacity: no spill-over leg
    return c


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _assert_rows_equal(got, ref, rows=None, what=""):
    """got[k][rows] (maps: [6, nvox] -> columns) bit-equal to ref[k] for every output"""
    for k in FIELDS:
        g, r = _np(got[k]), _np(ref[k])
        if rows is not None:
            g = g[:, rows] if k == "maps" else g[rows]
        g = g.reshape(r.shape)
        if not np.array_equal(g, r):
            if g.ndim == 2 and k != "maps":
                bad = ~np.all(g == r, axis=1)
            elif k == "maps":
                bad = ~np.all(g == r, axis=0)
            else:
                bad = g != r
            raise AssertionError("%s: %s differs in %d of %d voxels (first at %s)" % (what, k, int(bad.sum()), bad.size, np.nonzero(bad)[0][:8]))


def _make_plan(pkg, synth, nte, nt2, pen):
    T2s = synth.t2_grid(nt2)
    plan = pkg.Met2Plan(nte, nt2, 1, device=0)
    plan.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, np.array([150.0]), 3000.0).set_penalty(pen, T2s)
    return plan, T2s


def _broad(nvox, seed, wide):
    """lobes broader than make_voxels' defaults: more voxels whose passive set outgrows the first kernel's LDS capacity"""
    r = np.random.default_rng(seed)
    if wide:
        return dict(sm=r.uniform(5.0, 12.0, nvox), sie=r.uniform(30.0, 80.0, nvox), T2ie=r.uniform(60.0, 150.0, nvox))
    return dict(sm=r.uniform(3.0, 8.0, nvox), sie=r.uniform(15.0, 40.0, nvox))


def _fit(plan, method, data):
    return plan.fit(method, data, want_lambda=True)


def find_queued(plan, method, data, idx, group=64):
    """The voxels among data[idx] that the first kernel queues for the spill-over kernel.  Whether a voxel is queued is decided by the first
    kernel alone (its own path at the plan's fixed capacity), so the spill count of a fit of any sub-list counts the queued voxels in it: groups
    of `group` voxels, bisected where the count is neither 0 nor all."""
    import torch

    def count(ix):
        plan.fit(method, data[torch.as_tensor(ix, device=data.device)].contiguous(), want_sig=False, want_maps=False, want_status=False)
        return plan.last_spill_count()
    found = []

    def split(ix, c):
        if c == 0:
            return
        if c == len(ix):
            found.extend(ix)
            return
        h = len(ix) // 2
        c1 = count(ix[:h])
        split(ix[:h], c1)
        split(ix[h:], c - c1)
    idx = np.asarray(idx)
    for s in range(0, idx.size, group):
        g = idx[s:s + group]
        split(g, count(g))
    return np.sort(np.asarray(found, dtype=np.int64))


# (nte, nt2, method, penalty): 48 x 120 is two bins per lane, capacity 71 in the first kernel; 32 x 60 one bin per lane, capacity 50.
# X2/I at 48 x 120: the plan-level seed's passive set (75 bins at 150 degrees) lies above the first kernel's capacity and within nT2.
CASES = [(48, 120, "X2", "L2"), (48, 120, "X2", "I"), (48, 120, "GCV", "L2"), (48, 120, "L_curve", "L1"), (32, 60, "X2", "L2")]
NLONG = {120: 16384, 60: 65536}        # long lists: measured ~40 % queued at 48 x 120 (broad lobes), ~9 % at 32 x 60 (broader ones)
NSHORT = 256
NSEARCH = {120: 512, 60: 1024}         # the prefix of the long list searched for queued voxels


class _Case:
    def __init__(self, pkg, synth, torch, key):
        nte, nt2, method, pen = key
        self.key, self.method, self.pen = key, method, pen
        self.plan, self.T2s = _make_plan(pkg, synth, nte, nt2, pen)
        n = NLONG[nt2]
        self.data, _, _ = synth.make_voxels(n, nte=nte, seed=20261016 + nt2, device="cuda:0", params=_broad(n, 7 + nt2, nt2 <= 64))
        self.long = _fit(self.plan, method, self.data)
        torch.cuda.synchronize()
        self.ntail = self.plan.last_spill_count()
        self.carve_long = _long_premise(self.plan, method, n, self.ntail)
        self._queued = None

    def queued(self):
        if self._queued is None:
            q = find_queued(self.plan, self.method, self.data, np.arange(NSEARCH[self.plan.n_t2]))
            self._queued = q[:NSHORT]
        return self._queued


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    host = importlib.import_module(PKG + ".host")
    cache = {}

    def case(key):
        if key not in cache:
            cache[key] = _Case(pkg, synth, torch, key)
        return cache[key]
    yield dict(torch=torch, pkg=pkg, synth=synth, host=host, case=case)
    for c in cache.values():
        c.plan.close()


def _ids(c):
    return "%dx%d-%s-%s" % c


def _seed_set_size(oracle, plan, pen, T2s, lam):
    """bins of the plan-level seed (fit_kernel.hpp, seed_kernel): the canonical two-peak spectrum through the dictionary, solved at the first
    Brent abscissa by the oracle's restatement of the same NNLS-Tikhonov problem -- the passive set of the unique minimiser"""
    n = plan.n_t2
    D = plan.get_dictionary()[:, :, 0]
    u = np.arange(n) / (n - 1.0)
    xc = 0.15 * np.exp(-0.5 * ((u - 0.13) / 0.05) ** 2) + 0.85 * np.exp(-0.5 * ((u - 0.39) / 0.05) ** 2)
    b = D @ xc
    x = oracle.nnls_tik(D, b / b[0], oracle.penalty(n, pen, T2s), lam)
    return int((x > 0).sum())


@pytest.mark.parametrize("key", CASES, ids=_ids)
def test_queued_voxels_short_queue_equals_long_queue(env, oracle, key):
    """The first NSHORT voxels of a long list (long queue: the first kernel's LDS layout in the spill-over kernel, capacity k2 < nT2), fitted on
    their own (queue <= grid: one wave per workgroup at capacity nT2), give the same bits; so does the long list through met2_fit_host in blocks
    of 4 096 voxels and in the blocks it picks itself."""
    torch, host = env["torch"], env["host"]
    c = env["case"](key)
    plan, method = c.plan, c.method
    sub = c.data[:NSHORT].contiguous()
    short = _fit(plan, method, sub)
    torch.cuda.synchronize()
    ntail_s = plan.last_spill_count()
    cs = _short_premise(plan, method, NSHORT, ntail_s)
    if method == "X2":
        gm = 0.5 * (3.0 - np.sqrt(5.0))
        kseed = _seed_set_size(oracle, plan, c.pen, c.T2s, gm * 10.0)      # x2_lo + g (x2_hi - x2_lo)
        print("MEASURED %s: seed set %d bins, first kernel's capacity %d" % (_ids(key), kseed, c.carve_long["k2"]))
        if c.pen == "I":             # the case of this parametrisation: a seed the first kernel does not use, that the short queue's capacity would hold
            assert c.carve_long["k2"] < kseed <= cs["k2"], (kseed, c.carve_long["k2"], cs["k2"])
    print("MEASURED %s: long list %d voxels, %d queued -> w2 %d, k2 %d; short list %d voxels, %d queued -> w2 %d, k2 %d"
          % (_ids(key), c.data.shape[0], c.ntail, c.carve_long["w2"], c.carve_long["k2"], NSHORT, ntail_s, cs["w2"], cs["k2"]))
    _assert_rows_equal(c.long, short, rows=slice(0, NSHORT), what="long vs short queue")
    d = c.data.cpu().numpy()
    for chunk in (4096, 0):
        got = host.fit_host(plan, method, d, want_lambda=True, chunk=chunk)
        _assert_rows_equal(got, c.long, what="fit_host chunk=%d vs plan.fit" % chunk)


@pytest.mark.parametrize("key", CASES, ids=_ids)
def test_queued_voxels_against_the_oracle_at_both_capacities(env, oracle, key):
    """The voxels that actually take the spill-over kernel, found by find_queued, against the oracle on the plan's dictionary: as fitted in the
    long queue (capacity k2 < nT2, the spill-over legs running) and in a short one (capacity nT2)."""
    torch = env["torch"]
    c = env["case"](key)
    plan, method = c.plan, c.method
    q = c.queued()
    assert q.size >= 32, q.size
    short = _fit(plan, method, c.data[torch.as_tensor(q, device="cuda:0")].contiguous())
    torch.cuda.synchronize()
    _short_premise(plan, method, q.size, plan.last_spill_count())
    assert plan.last_spill_count() == q.size                  # every one of them queued, on its own too
    D = np.ascontiguousarray(np.transpose(plan.get_dictionary(), (2, 0, 1)))
    L = oracle.penalty(plan.n_t2, c.pen, c.T2s)
    d = c.data.cpu().numpy()[q]
    lam_grid = np.zeros(50)                                   # the plan's L-curve grid (plan.py, Met2Plan.__init__)
    lam_grid[1:] = np.logspace(np.log10(1e-8), np.log10(10.0), num=49, endpoint=True, base=10.0)
    fo, _, _, _, lo = oracle.fit_batch(method, D, L, d, np.zeros(q.size), np.ones(q.size), lambda_reg=lam_grid, nthreads=NTHREADS, want_lambda=True)
    for what, out, rows in (("long queue", c.long, q), ("short queue", short, None)):
        f = _np(out["fsol"]); lam = _np(out["lam"])
        if rows is not None:
            f, lam = f[rows], lam[rows]
        e = relmax_rows(f, fo)
        over = e >= TOL
        mwf = lambda x: np.sum(x[:, c.T2s <= 40.0], axis=1) / np.maximum(np.sum(x, axis=1), 1e-300)
        dm = np.abs(mwf(f) - mwf(fo))
        print("MEASURED %s %s: %d queued voxels vs oracle, %d over 1e-5, max %.2e, median |dMWF| %.2e, max |dlam| %.2e"
              % (_ids(key), what, q.size, int(over.sum()), e.max(), np.median(dm), np.max(np.abs(lam - lo))))
        if method == "GCV":          # the staircase objective: distributional (test_tail_parity.py:142)
            # HIP's lambda reaches a GCV value no higher than the oracle's in the same share of voxels (objective evaluated by the oracle at both)
            M = d / d[:, :1]
            dobj = np.array([np.diff(oracle.objective("GCV", D[0], M[v], L, np.array([lo[v], lam[v]])))[0] for v in range(q.size)])
            print("MEASURED %s %s: frac over 1e-5 %.3f, p99 |dMWF| %.2e, max |dMWF| %.2e, GCV(HIP) - GCV(oracle) median %.2e q90 %.2e, "
                  "HIP no worse in %.3f" % (_ids(key), what, over.mean(), np.quantile(dm, 0.99), dm.max(), np.median(dobj), np.quantile(dobj, 0.9),
                                            np.mean(dobj <= 0.0)))
            assert np.median(dobj) <= 1e-6 and np.quantile(dobj, 0.9) <= 0.11, (np.median(dobj), np.quantile(dobj, 0.9))
            # bounds as test_tail_parity.py derives them, from these voxels' measured values (their spectra are broader than the tail fixtures':
            # more of them sit on the staircase): the rate over 1e-5 (measured 158 of 214) with a one-sided 99 % binomial margin, the MWF
            # differences (measured median 1.9e-6, p99 1.6e-3, max 2.5e-3) at ~3x
            assert over.sum() <= binom99(0.74, over.size), (int(over.sum()), over.size)
            assert np.median(dm) <= 6e-6 and np.quantile(dm, 0.99) <= 5e-3 and dm.max() <= 1e-2, (np.median(dm), np.quantile(dm, 0.99), dm.max())
        elif method == "L_curve":    # the corner of the same grid: identical lambda, spectra at rounding level
            assert not over.any() and np.array_equal(lam, lo), (e.max(), int((lam != lo).sum()))
        else:                        # X2: Brent ties at the tail suite's rate, each a point of fminbound's own tolerance interval
            assert int(over.sum()) <= binom99(6e-5, q.size), (int(over.sum()), e[over])
            assert np.all(np.abs(lam - lo)[over] <= 1e-5), (lam[over], lo[over])


def test_lcurve_beyond_the_record_cap(env):
    """L-curve at 48 x 120 (two bins per lane): a launch whose queue exceeds lc_cap (the records of saved sweep states, met2_hip.hip fit_impl)
    gives every voxel -- and every tiled copy of a queued voxel -- the bits of its fit in a short list, where it certainly resumes; two runs are
    bit-equal, and so is met2_fit_host at two block sizes."""
    torch, host = env["torch"], env["host"]
    c = env["case"]((48, 120, "L_curve", "L1"))
    plan = c.plan
    q = c.queued()
    assert q.size >= 32, q.size
    head = 512
    nvox = 8192
    idx = np.concatenate([np.arange(head), np.resize(q, nvox - head)])
    data = c.data[torch.as_tensor(idx, device="cuda:0")].contiguous()
    a = _fit(plan, "L_curve", data)
    torch.cuda.synchronize()
    nq = plan.last_spill_count()
    lc_cap = min(nvox, 262144, max(4096, nvox // 16))        # fit_impl's record count for this launch
    print("MEASURED L-curve beyond the record cap: %d voxels, %d queued, lc_cap %d" % (nvox, nq, lc_cap))
    assert nq > lc_cap and nq > nvox // 16 and nq >= nvox - head, (nq, lc_cap)
    _long_premise(plan, "L_curve", nvox, nq)
    # each voxel in a short list: the first `head` voxels in lists of NSHORT, the queued ones on their own
    ref = {k: [] for k in FIELDS}
    for s in range(0, head, NSHORT):
        o = _fit(plan, "L_curve", c.data[s:s + NSHORT].contiguous())
        torch.cuda.synchronize()
        _short_premise(plan, "L_curve", NSHORT, plan.last_spill_count())
        for k in FIELDS:
            ref[k].append(o[k])
    oq = _fit(plan, "L_curve", c.data[torch.as_tensor(q, device="cuda:0")].contiguous())
    torch.cuda.synchronize()
    _short_premise(plan, "L_curve", q.size, plan.last_spill_count())
    pos = np.resize(np.arange(q.size), nvox - head)
    pos_t = torch.as_tensor(pos, device="cuda:0")
    for k in FIELDS:
        tail = oq[k][:, pos_t] if k == "maps" else oq[k][pos_t]
        ref[k] = torch.cat(ref[k] + [tail], dim=-1 if k == "maps" else 0)
    _assert_rows_equal(a, ref, what="beyond lc_cap vs short lists")
    b = _fit(plan, "L_curve", data)
    _assert_rows_equal(b, a, what="second run")
    d = data.cpu().numpy()
    for chunk in (4096, 0):
        got = host.fit_host(plan, "L_curve", d, want_lambda=True, chunk=chunk)
        _assert_rows_equal(got, a, what="fit_host chunk=%d vs plan.fit" % chunk)


IV_CASES = [(nte, nt2, m, p) for nte, nt2 in ((48, 120), (32, 60)) for m, p in (("X2", "L2"), ("GCV", "L2"), ("BayesReg", "I"))]


@pytest.mark.parametrize("key", IV_CASES, ids=_ids)
def test_custom_intervals_many_voxels_per_wave(env, oracle, key):
    """Non-default lambda-search intervals send every fitted voxel through the spill-over kernel (all_queued).  16 384 voxels: all waves of the
    first kernel's layout, ~8 (48 x 120) or ~4-6 (32 x 60) voxels per wave through the not-inlined voxel routine and one global slot, at capacity
    k2 < nT2 (BayesReg at 32 x 60: the plan's capacity is nT2 already).  The first 256 equal a 256-voxel fit (capacity nT2), every voxel is FITTED, and a 512-voxel sample agrees with the oracle on the
    same intervals (test_round5.py's rules)."""
    torch, pkg, synth = env["torch"], env["pkg"], env["synth"]
    nte, nt2, method, pen = key
    plan, T2s = _make_plan(pkg, synth, nte, nt2, pen)
    plan.set_options(**dict(zip(IV_NAMES, INTERVALS)))
    nvox = 16384
    data, _, _ = synth.make_voxels(nvox, nte=nte, seed=20261017 + nt2, device="cuda:0")
    out = _fit(plan, method, data)
    torch.cuda.synchronize()
    nq = plan.last_spill_count()
    short = _fit(plan, method, data[:NSHORT].contiguous())
    torch.cuda.synchronize()
    nq_s = plan.last_spill_count()
    st = _np(out["status"])
    assert nq == nvox and nq_s == NSHORT, (nq, nq_s)                 # every fitted voxel went through the spill-over kernel (all_queued)
    cl = _long_premise(plan, method, nvox, nq, legs=not (method == "BayesReg" and nt2 <= 64))
    cs = _short_premise(plan, method, NSHORT, nq_s)
    print("MEASURED intervals %s: %d voxels -> w2 %d, k2 %d (%.1f voxels per wave); %d voxels -> w2 %d, k2 %d"
          % (_ids(key), nvox, cl["w2"], cl["k2"], nvox / (cl["grid"] * cl["w2"]), NSHORT, cs["w2"], cs["k2"]))
    assert np.all(st == 1), np.unique(st, return_counts=True)
    _assert_rows_equal(out, short, rows=slice(0, NSHORT), what="16 384 vs 256 voxels")
    ns = 512
    D = np.ascontiguousarray(np.transpose(plan.get_dictionary(), (2, 0, 1)))
    L = oracle.penalty(nt2, pen, T2s)
    d = data[:ns].cpu().numpy()
    fo, _, _, _, lo = oracle.fit_batch(method, D, L, d, np.zeros(ns), np.ones(ns), nthreads=NTHREADS, want_lambda=True, intervals=INTERVALS)
    f, lam = _np(out["fsol"])[:ns], _np(out["lam"])[:ns]
    e = relmax_rows(f, fo)
    lo_iv, hi_iv = {"X2": INTERVALS[0:2], "GCV": INTERVALS[2:4], "BayesReg": INTERVALS[4:6]}[method]
    print("MEASURED intervals %s vs oracle: n_over=%d of %d, max %.2e, max |dlam| %.2e, median |dlam| %.2e"
          % (_ids(key), int((e >= TOL).sum()), ns, e.max(), np.max(np.abs(lam - lo)), np.median(np.abs(lam - lo))))
    assert np.all((lam >= lo_iv) & (lam <= hi_iv))
    if method == "GCV":
        assert np.median(np.abs(lam - lo)) < 1e-2 * (hi_iv - lo_iv)
    else:
        assert int((e >= TOL).sum()) <= 1 and np.max(np.abs(lam - lo)) < 1e-4
    plan.close()


def test_bootstrap_two_bins_per_lane_split_equals_whole(env):
    """met2_fit_bootstrap at 48 x 120, X2/L2: one call whose replicate rows make a long spill-over queue equals the same voxels split into calls
    (voxel_id passed) whose queues are short -- stats, sigma and rep_status bit for bit (test_gpu_bootstrap.py checks this at 32 x 60, where no
    spill-over leg runs)."""
    torch, pkg, synth = env["torch"], env["pkg"], env["synth"]
    plan, _ = _make_plan(pkg, synth, 48, 120, "L2")
    nvox, B, seed, piece = 512, 16, 2 ** 33 + 5, 8
    data, _, _ = synth.make_voxels(nvox, nte=48, seed=20261018, device="cuda:0", params=_broad(nvox, 19, False))
    whole = plan.fit_bootstrap("X2", data, n_rep=B, seed=seed)
    torch.cuda.synchronize()
    nq = plan.last_spill_count()
    cl = _long_premise(plan, "X2", nvox * B, nq)
    parts, nq_max = [], 0
    for a in range(0, nvox, piece):
        parts.append(plan.fit_bootstrap("X2", data[a:a + piece].contiguous(), n_rep=B, seed=seed, voxel_id=np.arange(a, a + piece)))
        torch.cuda.synchronize()
        nq_max = max(nq_max, plan.last_spill_count())
    cs = _carve(plan, "X2", piece * B, nq_max)
    print("MEASURED bootstrap: whole call %d replicate rows, %d queued -> w2 %d, k2 %d; pieces of %d rows, at most %d queued -> w2 %d, k2 %d"
          % (nvox * B, nq, cl["w2"], cl["k2"], piece * B, nq_max, cs["w2"], cs["k2"]))
    assert nq_max > 0 and cs["w2"] == 1 and cs["k2"] == 120, cs
    for k in ("stats", "sigma", "rep_status"):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts], dim=-1)), k
    plan.close()
