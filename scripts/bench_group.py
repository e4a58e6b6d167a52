#!/usr/bin/env python3
"""Timing of the voxel-wise permutation test (met2_group_perm_stats, group.randomise) on the device, written to profiles/group_bench.json:
    python3 scripts/bench_group.py [--perms 5000] [--voxels 250000] [--subjects 32] [--reps 5] [--numpy-candidates 32] [--out FILE]
                                   [--tfce [--grid 96 112 96] [--numpy-seconds 60] [--device-only]] [--fstat [--grid 96 112 96]]
                                   [--vsm [--sigma 2.5] [--grid 96 112 96]] [--mass [--threshold 2.5] [--grid 96 112 96]]
The case: two groups of subjects / 2 (r = 2 model columns), seeded normal data with a group difference in 1 % of the voxels, `perms`
permutations drawn at random, one map.
  kernels     the launches of the whole set (ceil(perms / max_k) calls of the entry with t_ref and count, inputs resident on the device), between
              HIP events on the launch stream: the median of `reps` passes after a warm-up pass.  The work by the algorithm is 2 n (r + 1)
              flop per (permutation, voxel); it is set against the 78.6 TFLOP/s fp64 vector peak that bench.py uses.  That peak counts a fused
              multiply-add as two operations in one instruction; the entry's contract forbids fusing (the order of summation is pinned to what
              numpy reproduces), so a product and a sum are two instructions and the ceiling of this kernel is half that peak.
  randomise   group.randomise end to end (host clock: the design's partition, the permutation set, the weights, the copies, the launches,
              the sort and the search, the copies back): the median of `reps` calls after a warm-up call.
  numpy       the float64 restatement of the entry (tests/tools/group_numpy.py, the same loop) on this machine's 16 threads, the voxels split
              over the threads, for `numpy-candidates` candidates; the time for the whole set is that time scaled by perms / candidates (the
              work is linear in the candidates), and is marked as scaled.
With --tfce the same case is placed on a grid (--grid 96 112 96: the voxels are an ellipsoid's, trimmed to `voxels`) and the test is the TFCE
one (group.randomise(tfce=True): met2_group_perm_tfce in batches of at most 32 maps), written to profiles/group_tfce_bench.json:
  randomise   end to end with tfce=True, and beside it the t-only call on the same data: the median of `reps` calls after a warm-up call
  numpy       the restatement (tests/tools/tfce_numpy.py: scipy.ndimage.label per level) on 16 threads, one candidate per task, for as many
              candidates as are finished within --numpy-seconds (60); the whole set is that rate scaled, and is marked as scaled
  --device-only leaves the restatement out and makes one call: the form for a kernel trace of its own (rocprofv3 --kernel-trace --stats),
              from which the stages' shares of the kernel time are read (gp_stats: t; tf_union, tf_count, tf_sum: the levels).
With --fstat the test is the F-test of three groups (subjects split 11 / 11 / 10 at 32; r = 3 model columns, s = 2 contrast rows), written to
profiles/group_f_bench.json:
  kernels     the launches of the whole set through met2_group_perm_fstats, as above, and in the same run the t entry (met2_group_perm_stats,
              group 1 against group 2) at the same n, r, V and P: the yardstick.  The F kernel carries r sums per candidate, the t kernel r + 1.
  randomise   group.randomise(f_contrast=...) end to end, and with tfce=True on the grid (--grid; the voxels an ellipsoid's, as with --tfce)
With --vsm the test is the one on the pseudo-t (variance smoothing, --sigma 2.5 voxels: a radius of 8), on the grid of --tfce, written to
profiles/group_vsm_bench.json, everything measured in one run on one build:
  kernels     the whole set through met2_group_perm_vsm in voxel mode (batches of at most 32 candidates, the work space handed in), and beside
              it the plain t entry (met2_group_perm_stats, batches of 256) on the same data
  passes      the three smoothing passes alone (met2_masked_smooth without N on 32 maps of the cropped grid), per call; a pass reads and
              writes every cell once, 16 bytes per cell and pass, set against the 8 TB/s HBM peak that bench.py uses
  randomise   group.randomise(variance_smoothing=sigma) end to end, and beside it the plain call and the tfce=True call on the same data
With --mass the test is the cluster-mass one (MET2_TFCE_MODE_MASS, --threshold 2.5, connectivity 26) on the case and grid of --tfce, with the
cluster extent at the same threshold and connectivity in the same run as the yardstick, written to profiles/group_mass_bench.json:
  transform   met2_tfce alone on one batch of 32 t maps of the cropped grid (the device's own, observed and permuted), extent and mass, between
              HIP events: the level, union, (count, sum | add, spread, roots) and finish launches
  kernels     the whole set through met2_group_perm_tfce, extent and mass, as above
  randomise   group.randomise(cluster_threshold=h) and group.randomise(cluster_mass_threshold=h) end to end
A record, not a pass mark."""
import argparse
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
PKG = "multicomponent-t2-toolbox_amd"
FP64_VECTOR_PEAK = 78.6e12                                         # bench.py's FP64_VECTOR_PEAK_TFLOPS
HBM_PEAK_GBPS = 8000.0                                             # bench.py's HBM_PEAK_GBPS
THREADS = 16


def ellipsoid(grid, voxels):
    """the indices of the `voxels` grid voxels nearest the centre in the grid's own ellipsoidal metric, ascending"""
    axes = [(np.arange(m) - (m - 1) / 2.0) / (m / 2.0) for m in grid]
    d = (axes[0][:, None, None] ** 2 + axes[1][None, :, None] ** 2 + axes[2][None, None, :] ** 2).ravel()
    return np.sort(np.argpartition(d, voxels - 1)[:voxels])


def tfce_case(a, group, gn):
    import tfce_numpy as tn
    n, V, P, grid = a.subjects, a.voxels, a.perms, tuple(a.grid)
    at = ellipsoid(grid, V)
    g = np.repeat([1.0, 0.0], n // 2)
    X, c = np.stack([g, 1.0 - g], axis=1), np.array([1.0, -1.0])
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((n, V))
    centre = np.argsort(np.abs(at - at[V // 2]))[: V // 100]      # 1 % of the voxels around the middle one (runs of a few rows: small blobs)
    Y[: n // 2, centre] += 1.5
    kw = dict(n_perm=P, seed=0)
    sp = dict(tfce=True, grid=grid, at=at)
    out = group.randomise(Y, X, c, **kw, **sp)                      # warm-up
    if a.device_only:
        print(json.dumps({"perms": out["n_perm"], "dh": out["dh"], "tfce_crit": out["tfce_crit"]}))
        return
    t_s, tfce_s = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        group.randomise(Y, X, c, **kw)
        t1 = time.perf_counter()
        out = group.randomise(Y, X, c, **kw, **sp)
        t_s.append(t1 - t0)
        tfce_s.append(time.perf_counter() - t1)
    box, at_box = group._crop(grid, at)
    K = group._batch_for(box, V, 2 ** 30, out["n_perm"])

    perms = group.permutation_set(X, c, P, 0, "permute")
    W, _ = group.weights(X, c, perms)
    Yr, s0 = group.residualise(Y, X, c)
    t_start, done = time.perf_counter(), []

    def one(k):
        if time.perf_counter() - t_start > a.numpy_seconds:
            return None
        return float(tn.perm_spatial(Yr, s0, W[k:k + 1], box, at_box, "tfce", out["dh"], 0.5, 2.0, 6)["kmax"][0])
    with ThreadPoolExecutor(THREADS) as pool:
        done = [x for x in pool.map(one, range(min(W.shape[0], 4096))) if x is not None]
        numpy_s = time.perf_counter() - t_start
    same = bool(np.array_equal(np.array(done), out["tfce_max_dist"][:len(done)]))
    rec = {"case": {"perms": out["n_perm"], "voxels": V, "subjects": n, "grid": list(grid), "cropped_grid": list(box), "maps_per_launch": K,
                    "launches": 1 + (out["n_perm"] + K - 1) // K, "dh": out["dh"], "E": 0.5, "H": 2.0, "connectivity": 6},
           "randomise_tfce": {"seconds": float(np.median(tfce_s)), "all_s": tfce_s, "tfce_crit": out["tfce_crit"],
                              "voxels_p_tfce_fwe_le_0.05": int((out["p_tfce_fwe"] <= 0.05).sum()),
                              "voxels_p_fwe_le_0.05": int((out["p_fwe"] <= 0.05).sum())},
           "randomise_t_only": {"seconds": float(np.median(t_s)), "all_s": t_s},
           "numpy_float64": {"threads": THREADS, "candidates_timed": len(done), "seconds_timed": numpy_s,
                             "seconds_whole_set_scaled": numpy_s * out["n_perm"] / max(len(done), 1), "scaled": True,
                             "tfce_max_equal_to_device": same},
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    path = a.out if a.out != os.path.join(ROOT, "profiles", "group_bench.json") else os.path.join(ROOT, "profiles", "group_tfce_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def events_ms(fn, reps):
    """the times of `reps` passes of fn between HIP events, after a warm-up pass"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def fstat_case(a, group):
    n, V, P, grid = a.subjects, a.voxels, a.perms, tuple(a.grid)
    sizes = [-(-n // 3), -(-n // 3), n - 2 * -(-n // 3)]           # 32 -> 11 / 11 / 10
    g = np.repeat(np.arange(3), sizes)
    X = np.stack([(g == j).astype(np.float64) for j in range(3)], axis=1)
    fc = np.array([[1.0, -1.0, 0.0], [0.0, 1.0, -1.0]])
    c = fc[0]
    at = ellipsoid(grid, V)
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((n, V))
    centre = np.argsort(np.abs(at - at[V // 2]))[: V // 100]      # 1 % of the voxels around the middle one
    Y[np.ix_(g == 1, centre)] += 1.5
    Y[np.ix_(g == 2, centre)] -= 1.5
    dev = torch.device("cuda", 0)
    K = group.limits()["max_k"]

    perms = group.permutation_set(X, fc.T, P, 0, "permute")
    Wf, s, dof = group.weights_f(X, fc.T, perms)
    Yf, s0f = group.residualise(Y, X, fc.T)
    Wt, _ = group.weights(X, c, group.permutation_set(X, c, P, 0, "permute"))
    Yc, s0c = group.residualise(Y, X, c)
    P, r = Wf.shape[0], Wf.shape[1]
    assert Wt.shape == (P, r + 1, n)
    put = lambda x: torch.as_tensor(x, device=dev)
    Yft, sft, Wft, Yct, sct, Wtt = (put(x) for x in (Yf, s0f, Wf, Yc, s0c, Wt))
    obs_f, obs_t = (torch.empty(V, dtype=torch.float64, device=dev) for _ in range(2))
    md = torch.empty(P, dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int32, device=dev)
    scale = float(dof) / s
    group._launch_f(dev, Yft, sft, Wft[:1], s, scale, None, obs_f, md[:1], None)
    group._launch(dev, Yct, sct, r, Wtt[:1], False, None, obs_t, md[:1], None)

    def f_set():
        for k0 in range(0, P, K):
            group._launch_f(dev, Yft, sft, Wft[k0:k0 + K], s, scale, obs_f, None, md[k0:k0 + K], cnt)

    def t_set():
        for k0 in range(0, P, K):
            group._launch(dev, Yct, sct, r, Wtt[k0:k0 + K], False, obs_t, None, md[k0:k0 + K], cnt)

    f_ms, t_ms = events_ms(f_set, a.reps), events_ms(t_set, a.reps)
    f_ms2 = events_ms(f_set, a.reps)                                # once more after the t passes: the order of the two does not decide
    kw = dict(n_perm=P, seed=0)
    group.randomise(Y, X, f_contrast=fc, **kw)
    group.randomise(Y, X, f_contrast=fc, tfce=True, grid=grid, at=at, **kw)
    plain_s, tfce_s = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = group.randomise(Y, X, f_contrast=fc, **kw)
        t1 = time.perf_counter()
        out_s = group.randomise(Y, X, f_contrast=fc, tfce=True, grid=grid, at=at, **kw)
        plain_s.append(t1 - t0)
        tfce_s.append(time.perf_counter() - t1)
    med = lambda x: float(np.median(x))
    rec = {"case": {"perms": P, "voxels": V, "subjects": n, "groups": sizes, "r": r, "s": int(s), "dof": [int(s), int(dof)],
                    "launches": (P + K - 1) // K, "grid": list(grid)},
           "kernels_f": {"seconds": med(f_ms) * 1e-3, "all_ms": f_ms, "all_ms_after_the_t_passes": f_ms2, "flop": 2.0 * n * r * P * V,
                         "achieved_tflops": 2.0 * n * r * P * V / (med(f_ms) * 1e-3) / 1e12},
           "kernels_t_same_n_r_V_P": {"seconds": med(t_ms) * 1e-3, "all_ms": t_ms, "flop": 2.0 * n * (r + 1) * P * V,
                                      "achieved_tflops": 2.0 * n * (r + 1) * P * V / (med(t_ms) * 1e-3) / 1e12},
           "f_over_t": med(f_ms) / med(t_ms), "spread_of_the_passes_ms": {"f": max(f_ms) - min(f_ms), "t": max(t_ms) - min(t_ms)},
           "randomise_f": {"seconds": med(plain_s), "all_s": plain_s, "f_crit": out["f_crit"],
                           "voxels_p_fwe_le_0.05": int((out["p_fwe"] <= 0.05).sum())},
           "randomise_f_tfce": {"seconds": med(tfce_s), "all_s": tfce_s, "dh": out_s["dh"], "tfce_crit": out_s["tfce_crit"],
                                "voxels_p_tfce_fwe_le_0.05": int((out_s["p_tfce_fwe"] <= 0.05).sum())},
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    path = a.out if a.out != os.path.join(ROOT, "profiles", "group_bench.json") else os.path.join(ROOT, "profiles", "group_f_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def vsm_case(a, group):
    n, V, P, grid, sigma = a.subjects, a.voxels, a.perms, tuple(a.grid), a.sigma
    at = ellipsoid(grid, V)
    g = np.repeat([1.0, 0.0], n // 2)
    X, c = np.stack([g, 1.0 - g], axis=1), np.array([1.0, -1.0])
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((n, V))
    centre = np.argsort(np.abs(at - at[V // 2]))[: V // 100]      # 1 % of the voxels around the middle one
    Y[: n // 2, centre] += 1.5
    W, dof = group.weights(X, c, group.permutation_set(X, c, P, 0, "permute"))
    Yr, s0 = group.residualise(Y, X, c)
    P, r = W.shape[0], W.shape[1] - 1
    box, at_box = group._crop(grid, at)
    radius, taps = group.smoothing_taps(sigma)
    dev = torch.device("cuda", 0)
    put = lambda x: torch.as_tensor(x, device=dev)
    Yt, st, Wt, at_t = put(Yr), put(s0), put(W), put(at_box)
    K = group._vsm_batch_for(box, V, "voxel", 2 ** 30, P)
    work = torch.empty(group.vsm_work_bytes(K, box, V, "voxel"), dtype=torch.uint8, device=dev)
    obs = torch.empty(V, dtype=torch.float64, device=dev)
    md = torch.empty(P, dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int32, device=dev)
    vsm = lambda Wk, ref, first, km, count: group._launch_vsm(dev, Yt, st, r, Wk, False, box, at_t, "voxel", 1.0, 0.5, 2.0, 6, radius, taps, ref,
                                                              first, km, count, work)
    vsm(Wt[:1], None, obs, md[:1], None)
    t_obs = torch.empty(V, dtype=torch.float64, device=dev)
    group._launch(dev, Yt, st, r, Wt[:1], False, None, t_obs, md[:1], None)
    Kt = group.limits()["max_k"]

    def vsm_set():
        for k0 in range(0, P, K):
            vsm(Wt[k0:k0 + K], obs, None, md[k0:k0 + K], cnt)

    def t_set():
        for k0 in range(0, P, Kt):
            group._launch(dev, Yt, st, r, Wt[k0:k0 + Kt], False, t_obs, None, md[k0:k0 + Kt], cnt)

    G = int(np.prod(box))
    maps = torch.rand((K, G), dtype=torch.float64, device=dev)
    out = torch.empty_like(maps)
    mask = torch.zeros(G, dtype=torch.uint8, device=dev)
    mask[at_t.long()] = 1
    ping = torch.empty(group.vsm_work_bytes(K, box), dtype=torch.uint8, device=dev)
    import ctypes as C
    lib = importlib.import_module(PKG + "._lib")
    targs, dims = group._taps_args(radius, taps), (C.c_int32 * 3)(*box)

    def passes():
        lib.check(lib.lib().met2_masked_smooth(0, K, dims, maps.data_ptr(), mask.data_ptr(), *targs, out.data_ptr(), None, ping.data_ptr(),
                                               ping.numel(), torch.cuda.current_stream(dev).cuda_stream))

    vsm_ms, t_ms, pass_ms = events_ms(vsm_set, a.reps), events_ms(t_set, a.reps), events_ms(passes, a.reps)
    kw = dict(n_perm=P, seed=0)
    sp = dict(grid=grid, at=at)
    group.randomise(Y, X, c, variance_smoothing=sigma, **kw, **sp)
    group.randomise(Y, X, c, tfce=True, **kw, **sp)
    plain_s, vsm_s, tfce_s = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        group.randomise(Y, X, c, **kw)
        t1 = time.perf_counter()
        res = group.randomise(Y, X, c, variance_smoothing=sigma, **kw, **sp)
        t2 = time.perf_counter()
        res_t = group.randomise(Y, X, c, tfce=True, **kw, **sp)
        plain_s.append(t1 - t0)
        vsm_s.append(t2 - t1)
        tfce_s.append(time.perf_counter() - t2)
    med = lambda x: float(np.median(x))
    pass_bytes = 3 * 16.0 * K * G
    rec = {"case": {"perms": P, "voxels": V, "subjects": n, "r": r, "grid": list(grid), "cropped_grid": list(box), "sigma_vox": sigma,
                    "radius": list(radius), "maps_per_launch": K, "launches": (P + K - 1) // K},
           "kernels_vsm_voxel": {"seconds": med(vsm_ms) * 1e-3, "all_ms": vsm_ms},
           "kernels_t_same_data": {"seconds": med(t_ms) * 1e-3, "all_ms": t_ms, "maps_per_launch": Kt},
           "vsm_over_t": med(vsm_ms) / med(t_ms),
           "smoothing_passes": {"maps": K, "cells_per_map": G, "seconds_three_passes": med(pass_ms) * 1e-3, "all_ms": pass_ms,
                                "bytes_three_passes": pass_bytes, "achieved_gb_per_s": pass_bytes / (med(pass_ms) * 1e-3) / 1e9,
                                "hbm_peak_gb_per_s": HBM_PEAK_GBPS, "share_of_hbm_peak": pass_bytes / (med(pass_ms) * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                                "note": "16 bytes per cell and pass by the algorithm; the halo's re-reads are not counted"},
           "randomise_vsm": {"seconds": med(vsm_s), "all_s": vsm_s, "t_crit": res["t_crit"], "voxels_p_fwe_le_0.05": int((res["p_fwe"] <= 0.05).sum())},
           "randomise_t_only": {"seconds": med(plain_s), "all_s": plain_s},
           "randomise_tfce": {"seconds": med(tfce_s), "all_s": tfce_s, "voxels_p_tfce_fwe_le_0.05": int((res_t["p_tfce_fwe"] <= 0.05).sum()),
                              "voxels_p_fwe_le_0.05": int((res_t["p_fwe"] <= 0.05).sum())},
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    path = a.out if a.out != os.path.join(ROOT, "profiles", "group_bench.json") else os.path.join(ROOT, "profiles", "group_vsm_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def mass_case(a, group):
    n, V, P, grid, h, conn = a.subjects, a.voxels, a.perms, tuple(a.grid), a.threshold, 26
    at = ellipsoid(grid, V)
    g = np.repeat([1.0, 0.0], n // 2)
    X, c = np.stack([g, 1.0 - g], axis=1), np.array([1.0, -1.0])
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((n, V))
    centre = np.argsort(np.abs(at - at[V // 2]))[: V // 100]      # 1 % of the voxels around the middle one
    Y[: n // 2, centre] += 1.5
    W, dof = group.weights(X, c, group.permutation_set(X, c, P, 0, "permute"))
    Yr, s0 = group.residualise(Y, X, c)
    P, r = W.shape[0], W.shape[1] - 1
    box, at_box = group._crop(grid, at)
    dev = torch.device("cuda", 0)
    put = lambda x: torch.as_tensor(x, device=dev)
    Yt, st, Wt, at_t = put(Yr), put(s0), put(W), put(at_box)
    K = group._batch_for(box, V, 2 ** 30, P)
    work = torch.empty(group.tfce_work_bytes(K, box, V), dtype=torch.uint8, device=dev)
    md = torch.empty(P, dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int32, device=dev)
    obs = {m: torch.empty(V, dtype=torch.float64, device=dev) for m in ("extent", "mass")}
    entry = lambda m, Wk, ref, first, km, count: group._launch_spatial(dev, Yt, st, r, Wk, box, at_t, m, h, 1.0, 1.0, conn, ref, first, km, count, work)
    for m in obs:
        entry(m, Wt[:1], None, obs[m], md[:1], None)

    def whole_set(m):
        for k0 in range(0, P, K):
            entry(m, Wt[k0:k0 + K], obs[m], None, md[k0:k0 + K], cnt)

    # one batch of t maps for the transform alone: the device's own t of the first K candidates, scattered to the cropped grid
    import ctypes as C
    lib = importlib.import_module(PKG + "._lib")
    G = int(np.prod(box))
    t_first = torch.empty(V, dtype=torch.float64, device=dev)
    maps = torch.zeros((K, G), dtype=torch.float64, device=dev)
    mask = torch.zeros(G, dtype=torch.uint8, device=dev)
    mask[at_t.long()] = 1
    for k in range(K):
        group._launch(dev, Yt, st, r, Wt[k:k + 1], False, None, t_first, md[:1], None)
        maps[k, at_t.long()] = t_first
    out, km = torch.empty_like(maps), torch.empty(K, dtype=torch.float64, device=dev)
    twork = torch.empty(group.tfce_work_bytes(K, box), dtype=torch.uint8, device=dev)
    dims = (C.c_int32 * 3)(*box)

    def transform(m):
        lib.check(lib.lib().met2_tfce(0, K, dims, maps.data_ptr(), mask.data_ptr(), group.MODES[m], float(h), 1.0, 1.0, conn, out.data_ptr(),
                                      km.data_ptr(), twork.data_ptr(), twork.numel(), torch.cuda.current_stream(dev).cuda_stream))

    tr_ms = {m: events_ms(lambda m=m: transform(m), a.reps) for m in ("extent", "mass", "extent")}     # the extent last as well: the order does not decide
    members = int((maps >= h).sum().item())
    set_ms = {m: events_ms(lambda m=m: whole_set(m), a.reps) for m in ("extent", "mass")}
    kw = dict(n_perm=P, seed=0, grid=grid, at=at, cluster_connectivity=conn)
    group.randomise(Y, X, c, cluster_threshold=h, **kw)
    group.randomise(Y, X, c, cluster_mass_threshold=h, **kw)
    ext_s, mass_s = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res_e = group.randomise(Y, X, c, cluster_threshold=h, **kw)
        t1 = time.perf_counter()
        res_m = group.randomise(Y, X, c, cluster_mass_threshold=h, **kw)
        ext_s.append(t1 - t0)
        mass_s.append(time.perf_counter() - t1)
    med = lambda x: float(np.median(x))
    rec = {"case": {"perms": P, "voxels": V, "subjects": n, "r": r, "grid": list(grid), "cropped_grid": list(box), "threshold": h,
                    "connectivity": conn, "maps_per_launch": K, "launches": (P + K - 1) // K, "members_in_the_transform_batch": members},
           "transform_extent": {"seconds": med(tr_ms["extent"]) * 1e-3, "all_ms": tr_ms["extent"]},
           "transform_mass": {"seconds": med(tr_ms["mass"]) * 1e-3, "all_ms": tr_ms["mass"]},
           "transform_mass_over_extent": med(tr_ms["mass"]) / med(tr_ms["extent"]),
           "kernels_extent": {"seconds": med(set_ms["extent"]) * 1e-3, "all_ms": set_ms["extent"]},
           "kernels_mass": {"seconds": med(set_ms["mass"]) * 1e-3, "all_ms": set_ms["mass"]},
           "kernels_mass_over_extent": med(set_ms["mass"]) / med(set_ms["extent"]),
           "randomise_extent": {"seconds": med(ext_s), "all_s": ext_s, "cluster_crit": res_e["cluster_crit"],
                                "voxels_p_cluster_fwe_le_0.05": int((res_e["p_cluster_fwe"] <= 0.05).sum())},
           "randomise_mass": {"seconds": med(mass_s), "all_s": mass_s, "mass_crit": res_m["mass_crit"],
                              "voxels_p_mass_fwe_le_0.05": int((res_m["p_mass_fwe"] <= 0.05).sum())},
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    path = a.out if a.out != os.path.join(ROOT, "profiles", "group_bench.json") else os.path.join(ROOT, "profiles", "group_mass_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--perms", type=int, default=5000)
    ap.add_argument("--voxels", type=int, default=250000)
    ap.add_argument("--subjects", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-candidates", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_bench.json"))
    ap.add_argument("--tfce", action="store_true")
    ap.add_argument("--grid", type=int, nargs=3, default=[96, 112, 96])
    ap.add_argument("--numpy-seconds", type=float, default=60.0)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--fstat", action="store_true")
    ap.add_argument("--vsm", action="store_true")
    ap.add_argument("--sigma", type=float, default=2.5)
    ap.add_argument("--mass", action="store_true")
    ap.add_argument("--threshold", type=float, default=2.5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a GPU"
    group = importlib.import_module(PKG + ".group")
    import group_numpy as gn
    if a.fstat:
        return fstat_case(a, group)
    if a.vsm:
        return vsm_case(a, group)
    if a.mass:
        return mass_case(a, group)
    if a.tfce:
        return tfce_case(a, group, gn)
    n, V, P = a.subjects, a.voxels, a.perms
    g = np.repeat([1.0, 0.0], n // 2)
    X, c = np.stack([g, 1.0 - g], axis=1), np.array([1.0, -1.0])
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((n, V))
    Y[: n // 2, : V // 100] += 1.5
    perms = group.permutation_set(X, c, P, 0, "permute")
    W, dof = group.weights(X, c, perms)
    Yr, s0 = group.residualise(Y, X, c)
    P, r, K = W.shape[0], W.shape[1] - 1, group.limits()["max_k"]
    flop = 2.0 * n * (r + 1) * P * V

    dev = torch.device("cuda", 0)
    Yt, st, Wt = (torch.as_tensor(x, device=dev) for x in (Yr, s0, W))
    t_obs = torch.empty(V, dtype=torch.float64, device=dev)
    md = torch.empty(P, dtype=torch.float64, device=dev)
    cnt = torch.zeros(V, dtype=torch.int32, device=dev)
    group._launch(dev, Yt, st, r, Wt[:1], False, None, t_obs, md[:1], None)

    def whole_set():
        for k0 in range(0, P, K):
            group._launch(dev, Yt, st, r, Wt[k0:k0 + K], False, t_obs, None, md[k0:k0 + K], cnt)

    whole_set()
    torch.cuda.synchronize()
    kernel_ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        whole_set()
        e1.record()
        e1.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
    kernel_s = float(np.median(kernel_ms)) * 1e-3

    group.randomise(Y, X, c, n_perm=P, seed=0)
    total_s = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = group.randomise(Y, X, c, n_perm=P, seed=0)
        total_s.append(time.perf_counter() - t0)

    Kn = min(a.numpy_candidates, P)
    edges = np.linspace(0, V, THREADS + 1).astype(int)
    part = lambda i: gn.perm_stats(Yr[:, edges[i]:edges[i + 1]], s0[edges[i]:edges[i + 1]], W[:Kn], False, None, np.float64)["kmax"]
    with ThreadPoolExecutor(THREADS) as pool:
        t0 = time.perf_counter()
        parts = list(pool.map(part, range(THREADS)))
        numpy_s = time.perf_counter() - t0
    same = bool(np.array_equal(np.max(np.stack(parts), axis=0), md[:Kn].cpu().numpy()))

    rec = {"case": {"perms": P, "voxels": V, "subjects": n, "r": r, "dof": dof, "launches": (P + K - 1) // K, "maps": 1},
           "kernels": {"seconds": kernel_s, "all_ms": kernel_ms, "flop": flop, "achieved_tflops": flop / kernel_s / 1e12,
                       "share_of_fp64_vector_peak": flop / kernel_s / FP64_VECTOR_PEAK, "peak_tflops": FP64_VECTOR_PEAK / 1e12,
                       "note": "the peak counts a fused multiply-add; the entry may not fuse, so its ceiling is half the peak"},
           "randomise": {"seconds": float(np.median(total_s)), "all_s": total_s, "voxels_p_fwe_le_0.05": int((out["p_fwe"] <= 0.05).sum()),
                         "t_crit": out["t_crit"]},
           "numpy_float64": {"threads": THREADS, "candidates_timed": Kn, "seconds_timed": numpy_s, "seconds_whole_set_scaled": numpy_s * P / Kn,
                             "scaled": Kn != P, "kmax_equal_to_device": same},
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
