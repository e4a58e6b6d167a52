"""Round 5: the lambda-search intervals in met2_options (ABI 6), the spill-over kernel's carving, the host entry's interleave,
and the multi-device paths that only run on a box with two GPUs."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from conftest import relmax_rows

PKG = "multicomponent-t2-toolbox_amd"
gpu = pytest.mark.gpu
TOL = 1e-5

# (x2_lo, x2_hi, gcv_lo, gcv_hi, bayes_lo, bayes_hi): none of them the reference's literals
INTERVALS = (0.05, 30.0, 1e-6, 4.0, 1e-6, 3.5)


def _problem(nvox, seed):
    synth = importlib.import_module(PKG + ".synth")
    nte, nt2 = 32, 60
    T2s = synth.t2_grid(nt2); T1s = 1000.0 * np.ones(nt2)
    data, _, _ = synth.make_voxels(nvox, nte=nte, seed=seed, device="cpu")
    return nte, nt2, T2s, T1s, np.asarray(data, dtype=np.float64)


def test_oracle_intervals_move_the_search(oracle):
    """The checker's own switch (met2o_set_intervals): with an interval that excludes the default solution the returned lambda sits inside the
    new interval, and resetting gives the reference's literals back."""
    nte, nt2, T2s, T1s, data = _problem(16, 5)
    D = oracle.dictionary_fa_major(nt2, T2s, T1s, nte, 10.0, np.array([150.0]), 3000.0)
    L = oracle.penalty(nt2, "L2", T2s)
    z, o = np.zeros(16), np.ones(16)
    f0, _, _, _, lam0 = oracle.fit_batch("X2", D, L, data, z, o, want_lambda=True)
    f1, _, _, _, lam1 = oracle.fit_batch("X2", D, L, data, z, o, want_lambda=True, intervals=(20.0, 30.0, 1e-8, 10.0, 1e-8, 2.0))
    f2, _, _, _, lam2 = oracle.fit_batch("X2", D, L, data, z, o, want_lambda=True)
    assert np.all((lam1 >= 20.0) & (lam1 <= 30.0)) and np.all(lam0 < 10.0)
    assert np.array_equal(lam0, lam2) and np.array_equal(f0, f2)


@gpu
@pytest.mark.parametrize("method,pen", [("X2", "L2"), ("GCV", "I"), ("BayesReg", "I")])
def test_lambda_search_intervals_from_the_options(method, pen):
    """met2_options.x2_lo .. bayes_hi (algorithms.py:219, :280, bayesian_interpolation.py:101): a fit on non-default intervals equals the
    oracle's on the same intervals -- seeds and BayesReg's factor tables rebuilt for them -- and differs from the default fit."""
    import torch
    from oracle import oracle
    oracle.build()
    pkg = importlib.import_module(PKG)
    nvox = 256
    nte, nt2, T2s, T1s, data = _problem(nvox, 11)
    plan = pkg.Met2Plan(nte, nt2, 1)
    plan.build_dictionary_epg(T2s, T1s, 10.0, np.array([150.0]), 3000.0).set_penalty(pen, T2s)
    d = torch.as_tensor(data, device="cuda")
    base = plan.fit(method, d, want_lambda=True)["lam"].cpu().numpy()
    names = ("x2_lo", "x2_hi", "gcv_lo", "gcv_hi", "bayes_lo", "bayes_hi")
    plan.set_options(**dict(zip(names, INTERVALS)))
    assert tuple(plan.get_options(*names)[k] for k in names) == INTERVALS
    out = plan.fit(method, d, want_lambda=True)
    lam = out["lam"].cpu().numpy()
    lo, hi = {"X2": INTERVALS[0:2], "GCV": INTERVALS[2:4], "BayesReg": INTERVALS[4:6]}[method]
    assert np.all((lam >= lo) & (lam <= hi))
    assert not np.array_equal(lam, base)
    D = np.ascontiguousarray(np.transpose(plan.get_dictionary(), (2, 0, 1)))
    Lm = oracle.penalty(nt2, pen, T2s)
    fs, _, _, _, lam_o = oracle.fit_batch(method, D, Lm, data, np.zeros(nvox), np.ones(nvox), nthreads=8, want_lambda=True, intervals=INTERVALS)
    e = relmax_rows(out["fsol"].cpu().numpy(), fs)
    print("MEASURED intervals %s/%s: n_over=%d of %d, max %.2e, max |dlam| %.2e" % (method, pen, int((e >= TOL).sum()), nvox, e.max(), np.max(np.abs(lam - lam_o))))
    if method == "GCV":       # the staircase objective: distributional
        assert np.median(np.abs(lam - lam_o)) < 1e-2 * (hi - lo)
    else:
        assert int((e >= TOL).sum()) <= 1 and np.max(np.abs(lam - lam_o)) < 1e-4      # (one Brent tie allowed, inside xtol)
    # back to the reference's literals: the first fit again, bit for bit (seeds and tables rebuilt)
    plan.set_options(x2_lo=0.0, x2_hi=10.0, gcv_lo=1e-8, gcv_hi=10.0, bayes_lo=1e-8, bayes_hi=2.0)
    again = plan.fit(method, d, want_lambda=True)["lam"].cpu().numpy()
    assert np.array_equal(again, base)
    with pytest.raises(Exception):
        plan.set_options(x2_lo=5.0, x2_hi=1.0)
    plan.close()


@gpu
def test_options_struct_of_an_earlier_abi_is_accepted():
    """A caller built against ABI 5 passes a shorter met2_options (struct_size says so): the plan takes what it carries and the
    reference's intervals for the rest."""
    import torch
    pkg = importlib.import_module(PKG)
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()

    class Options5(C.Structure):
        _fields_ = lib.Options._fields_[:9]
    o5 = Options5()
    full = lib.Options()
    L.met2_default_options(C.byref(full))
    C.memmove(C.byref(o5), C.byref(full), C.sizeof(Options5))
    o5.struct_size = C.sizeof(Options5)
    o5.x2_factor = 1.05
    h = C.c_void_p(0)
    create = L.met2_plan_create
    rc = create(C.byref(h), 32, 60, 1, C.cast(C.byref(o5), C.POINTER(lib.Options)))
    assert rc == 0, L.met2_last_error()
    got = lib.Options()
    assert L.met2_plan_get_options(h, C.byref(got)) == 0
    assert got.x2_factor == 1.05 and (got.x2_lo, got.x2_hi, got.gcv_lo, got.gcv_hi, got.bayes_lo, got.bayes_hi) == (0.0, 10.0, 1e-8, 10.0, 1e-8, 2.0)
    assert got.struct_size == C.sizeof(lib.Options)
    L.met2_plan_destroy(h)


def _plans(pkg, n, nfa=1, pen="L2", alphas=None, nte=32, nt2=60, device=0):
    synth = importlib.import_module(PKG + ".synth")
    T2s = synth.t2_grid(nt2); T1s = 1000.0 * np.ones(nt2)
    al = np.array([150.0]) if alphas is None else alphas
    out = []
    for i in range(n):
        p = pkg.Met2Plan(nte, nt2, len(al), device=device if np.isscalar(device) else device[i])
        p.build_dictionary_epg(T2s, T1s, 10.0, al, 3000.0).set_penalty(pen, T2s).set_t2_grid(T2s)
        out.append(p)
    return out


@gpu
def test_host_entry_strided_view_with_a_separate_fa_volume():
    """data = big[:, :n_te] (row pitch > n_te) together with an fa_data of another layout -- the two must reach the C entry with ONE
    pair of strides that is right for both.  Equal to the same call on compact copies."""
    import torch
    pkg = importlib.import_module(PKG)
    host = importlib.import_module(PKG + ".host")
    nvox, nte = 3000, 32
    _, _, _, _, d = _problem(nvox, 21)
    rng = np.random.default_rng(2)
    big = np.zeros((nvox, nte + 8)); big[:, :nte] = d; big[:, nte:] = rng.uniform(size=(nvox, 8)) * 1e3
    view = big[:, :nte]
    fa_vol = d * (1.0 + 0.01 * rng.standard_normal(d.shape))        # what the FA step sees: compact, C-ordered
    alphas = np.linspace(120.0, 180.0, 13)
    plan, = _plans(pkg, 1, alphas=alphas)
    a = host.fit_host(plan, "X2", view, estimate_fa=True, fa_data=fa_vol, want_lambda=True)
    b = host.fit_host(plan, "X2", np.ascontiguousarray(view), estimate_fa=True, fa_data=np.ascontiguousarray(fa_vol), want_lambda=True)
    for k in ("fsol", "sig", "reg", "lam", "fa_index", "maps", "status"):
        assert np.array_equal(a[k], b[k]), k
    plan.close()


@gpu
@pytest.mark.parametrize("layout", ["C", "F"])
def test_host_entry_deals_runs_of_4096_voxels_over_the_plans(layout):
    """Several plans: the voxel list is dealt in runs of 4 096 voxels (run j -> plan j mod n_plans), a plan's block being chunk / 4 096 of ITS runs
    moved by pitched copies.  Any number of plans, pinned or pageable arrays, C-ordered list or Fortran-ordered volume, a ragged tail: bit-equal
    to one plan over the whole list (and to the whole-block dealing of round 4, MET2_HOST_BLOCKS=1)."""
    import torch
    pkg = importlib.import_module(PKG)
    host = importlib.import_module(PKG + ".host")
    nvox = 5 * 4096 * 3 + 1234                                       # 15 whole runs and a ragged one
    _, _, _, _, d = _problem(nvox, 31)
    rng = np.random.default_rng(3)
    mask = rng.uniform(size=nvox) > 0.1
    data = d if layout == "C" else np.asfortranarray(d.reshape(nvox, 1, 1, 32))      # (Fortran order: echo-major, every echo one contiguous row of voxels)
    plans = _plans(pkg, 3, alphas=np.linspace(120.0, 180.0, 7))
    ref = host.fit_host(plans[0], "X2", data, mask=mask, estimate_fa=True, want_lambda=True)
    for n, chunk in ((2, 0), (3, 8192), (3, 5000)):
        got = host.fit_host(plans[:n], "X2", data, mask=mask, estimate_fa=True, want_lambda=True, chunk=chunk)
        for k in ("fsol", "sig", "reg", "lam", "fa_index", "maps", "status"):
            assert np.array_equal(got[k], ref[k]), (n, chunk, k)
    os.environ["MET2_HOST_BLOCKS"] = "1"
    try:
        got = host.fit_host(plans, "X2", data, mask=mask, estimate_fa=True, want_lambda=True, chunk=8192)
    finally:
        del os.environ["MET2_HOST_BLOCKS"]
    for k in ("fsol", "lam", "fa_index"):
        assert np.array_equal(got[k], ref[k]), k
    # pinned arrays: the DMA engines reach the caller's arrays themselves (pitched copies in both directions)
    pin = torch.from_numpy(np.ascontiguousarray(d)).pin_memory()
    got = host.fit_host(plans, "X2", pin.numpy(), mask=mask, estimate_fa=True, want_lambda=True, chunk=8192)
    ref_c = ref if layout == "C" else host.fit_host(plans[0], "X2", d, mask=mask, estimate_fa=True, want_lambda=True)
    for k in ("fsol", "sig", "reg", "lam", "fa_index", "maps", "status"):
        assert np.array_equal(got[k], ref_c[k]), ("pinned", k)
    for p in plans:
        p.close()


# ---- paths that need two devices: skipped on a one-GPU box, so the driver's GPU test tier stays green there; they run on the first multi-GPU lease
def _two_gpus():
    import torch
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


@gpu
def test_host_entry_over_two_devices_equals_one_fit():
    """met2_fit_host with one plan per DEVICE (motor:427-441 is one process): devices [0, 1], runs of 4 096 voxels dealt
    alternately, every device's copies over its own PCIe link -- bit-equal to one met2_fit on device 0."""
    if not _two_gpus():
        pytest.skip("needs two GPUs")
    import torch
    pkg = importlib.import_module(PKG)
    host = importlib.import_module(PKG + ".host")
    nvox = 9 * 4096 + 777
    _, _, _, _, d = _problem(nvox, 41)
    alphas = np.linspace(120.0, 180.0, 13)
    plans = _plans(pkg, 2, alphas=alphas, device=[0, 1])
    got = host.fit_host(plans, "X2", d, estimate_fa=True, want_lambda=True)
    assert got["plan_ms"].shape == (2,) and (got["plan_ms"] > 0).all()
    with torch.cuda.device(0):
        dd = torch.as_tensor(d, device="cuda:0")
        fa, _, _ = plans[0].fa_bruteforce(dd)
        ref = plans[0].fit("X2", dd, fa_index=fa, want_lambda=True)
    for k in ("fsol", "sig", "reg", "lam", "maps"):
        assert np.array_equal(got[k], ref[k].cpu().numpy()), k
    assert np.array_equal(got["fa_index"], fa.cpu().numpy())
    for p in plans:
        p.close()


_RCCL2_WORKER = r"""
import os, sys, importlib
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
pkg = importlib.import_module(%(pkg)r)
d = importlib.import_module(%(pkg)r + ".dist")
synth = importlib.import_module(%(pkg)r + ".synth")
rank, local, world = d.init(backend="nccl")                     # one process per GPU, RCCL over xGMI
assert world == 2 and dist.get_backend() == "nccl" and torch.cuda.current_device() == local
nte, nt2, nvox = 32, 60, 20000
T2s = synth.t2_grid(nt2)
plan = pkg.Met2Plan(nte, nt2, 1, device=local)
plan.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, np.array([150.0]), 3000.0).set_penalty("L2", T2s)
data, _, _ = synth.make_voxels(nvox, nte=nte, seed=11, device="cuda:%%d" %% local)
out, full = d.fit_sharded(lambda idx: plan.fit("X2", data[idx].contiguous()), nvox, gather=("fsol", "sig", "reg", "maps"))
torch.cuda.synchronize()
if rank == 0:
    ref = plan.fit("X2", data)
    assert full["fsol"].is_cuda and torch.equal(full["fsol"], ref["fsol"]) and torch.equal(full["maps"], ref["maps"]) and torch.equal(full["reg"], ref["reg"])
    print("RCCL2_OK")
else:
    assert full is None
dist.barrier(); dist.destroy_process_group()
"""


@gpu
def test_fit_sharded_over_a_two_rank_rccl_group(tmp_path):
    """dist.fit_sharded with two processes, one GPU each, backend nccl = RCCL: interleaved 4 096-voxel blocks, ONE gather of the packed outputs
    from device to device -- bit-equal to the unsharded fit on rank 0."""
    if not _two_gpus():
        pytest.skip("needs two GPUs")
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rccl2.py"
    script.write_text(_RCCL2_WORKER % {"root": root, "pkg": PKG})
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = str(29300 + os.getpid() % 200)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", port,
                        str(script)], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and "RCCL2_OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


@gpu
def test_lcurve_spill_over_goes_on_from_the_saved_sweep_state():
    """L-curve at two bins per lane: a voxel whose set outgrows the LDS capacity is queued with its sweep's state (log norms so far, kept states,
    the iterate in hand: fit_kernel.hpp, FitArgs::lc_save) and the spill-over kernel goes on from the grid point that overflowed.  Against the
    same library starting such voxels over (MET2_LC_RESTART, read at every fit): the same bits in every voxel.  Up to the grid point that
    overflowed both paths run the same solves with the same sums (the spill-over legs sum in the fast legs' order), so the log norms and kept
    states from there are the same bits; the corner's solve starts from a kept state (or the state in hand), and in every voxel measured the
    solves beyond the overflow -- the saved iterate re-factorised, against the sweep's factor carried along -- gave the same bits too
    (383 queued voxels here; 7 944 in tests/test_gpu_launch_context.py, 3 848 of them beyond the records)."""
    import torch
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    nte, nt2, nvox = 48, 120, 8192
    T2s = synth.t2_grid(nt2); T1s = 1000.0 * np.ones(nt2)
    plan = pkg.Met2Plan(nte, nt2, 1)
    plan.build_dictionary_epg(T2s, T1s, 10.0, np.array([150.0]), 3000.0).set_penalty("L1", T2s)
    data, _, _ = synth.make_voxels(nvox, nte=nte, seed=20260110, device="cuda")
    a = plan.fit("L_curve", data, want_lambda=True)
    n_spill = plan.last_spill_count()
    assert n_spill > 100, n_spill                     # ~5 % of the voxels at this shape
    os.environ["MET2_LC_RESTART"] = "1"
    try:
        b = plan.fit("L_curve", data, want_lambda=True)
        assert plan.last_spill_count() == n_spill
    finally:
        os.environ.pop("MET2_LC_RESTART", None)
    assert torch.equal(a["status"], b["status"]) and int((a["status"] > 0).sum()) == nvox
    assert torch.equal(a["lam"], b["lam"])
    fa_, fb_ = a["fsol"].cpu().numpy(), b["fsol"].cpu().numpy()
    rel = np.abs(fa_ - fb_).max(axis=1) / np.abs(fb_).max(axis=1)
    print("MEASURED L-curve resume vs restart: %d queued, max rel diff %.2e, differing voxels %d" % (n_spill, rel.max(), (rel > 0).sum()))
    assert torch.equal(a["fsol"], b["fsol"]) and torch.equal(a["maps"], b["maps"]) and torch.equal(a["reg"], b["reg"]), rel.max()


@gpu
def test_lcurve_saved_sweep_states_through_the_host_entry():
    """The L-curve's sweep-state records (FitArgs::lc_save) are sized per fit: through met2_fit_host a plan fits block after block (different sizes, the
    last one ragged) and two plans hold records of their own.  48 x 120, L1: bit-equal to one plan.fit over the whole list, and voxels were queued."""
    import torch
    pkg = importlib.import_module(PKG)
    host = importlib.import_module(PKG + ".host")
    synth = importlib.import_module(PKG + ".synth")
    nte, nt2, nvox = 48, 120, 3 * 4096 + 777
    T2s = synth.t2_grid(nt2); T1s = 1000.0 * np.ones(nt2)
    plans = []
    for _ in range(2):
        p = pkg.Met2Plan(nte, nt2, 1)
        p.build_dictionary_epg(T2s, T1s, 10.0, np.array([150.0]), 3000.0).set_penalty("L1", T2s)
        plans.append(p)
    data, _, _ = synth.make_voxels(nvox, nte=nte, seed=20260111, device="cuda")
    ref = plans[0].fit("L_curve", data, want_lambda=True)
    assert plans[0].last_spill_count() > 50
    d = data.cpu().numpy()
    for pl, chunk in ((plans[:1], 4096), (plans, 4096), (plans, 0)):
        got = host.fit_host(pl, "L_curve", d, want_lambda=True, chunk=chunk)
        for k in ("fsol", "sig", "reg", "lam", "maps", "status"):
            r = ref[k]
            r = r.cpu().numpy() if hasattr(r, "cpu") else r
            assert np.array_equal(np.asarray(got[k]).reshape(r.shape), r), (len(pl), chunk, k)
    for p in plans:
        p.close()
