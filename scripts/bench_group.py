#!/usr/bin/env python3
"""Timing of the voxel-wise permutation test (met2_group_perm_stats, group.randomise) on the device, written to profiles/group_bench.json:
    python3 scripts/bench_group.py [--perms 5000] [--voxels 250000] [--subjects 32] [--reps 5] [--numpy-candidates 32] [--out FILE]
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
THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--perms", type=int, default=5000)
    ap.add_argument("--voxels", type=int, default=250000)
    ap.add_argument("--subjects", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-candidates", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the benchmark needs a GPU"
    group = importlib.import_module(PKG + ".group")
    import group_numpy as gn
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
