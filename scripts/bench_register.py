#!/usr/bin/env python3
"""Timing of the registration on the device, written to profiles/register_bench.json:
    python3 scripts/bench_register.py [--shape 128 128 64] [--reps 20] [--voxel 1.0] [--threads 16] [--reg-reps 7] [--numpy-reps 3] [--out FILE]
1. One launch of the cost (met2_register_cost: the H2D copy of the transforms, the cost kernel and the final kernel) for K = 1, 16 and 64
   candidates, fixed and moving volumes of `shape`, the three measures (64 bins for corratio, one for the others, as register calls them), next to ONE order-1 met2_resample of the same grid measured in
   the same run, the calls alternating: the cost does the same gathers per candidate, plus a reduction.  Inputs resident on the device; times
   are medians of `reps` calls after a warm-up call, between HIP events on the launch stream.  The candidates are rotations of up to 10 degrees
   with shifts of a few voxels, as a search proposes them.
2. A whole registration (register.register, defaults) at 6 and 12 degrees of freedom of the tests' phantom sampled at `voxel` mm (1 mm:
   40 x 36 x 32 and 44 x 40 x 36 voxels), wall clock with the device costs and with the numpy restatement in fp64 (tests/tools/register_numpy.py)
   as cost_fn, its candidates dealt to `threads` threads, the pyramid on the CPU (scipy): after a warm-up the median of `reg-reps` device runs
   and of `numpy-reps` restatement runs, the two alternating, every single time kept beside it (a run is a fraction of a second).  Both runs take the same path unless a comparison ties
   in the last bits; the mean displacement from the true transform is given for both.
With --kinds mi nmi (any of the two) the mutual-information costs are measured instead, into profiles/register_mi_bench.json; the default output
is untouched:
1. One launch of met2_register_joint_cost (the H2D copy of the transforms, the table's memset, the histogram kernel and the final kernel) at
   64 x 64 bins for K = 1, 16 and 64, next to one launch of 'corratio' at 64 bins on the same inputs and candidates, the two alternating; the
   ratio of the medians is what the histogram costs on top of corratio's sampling.
2. One whole 6-dof registration per kind of the 1 mm phantom, device against the fp64 restatement (tests/tools/register_mi_numpy.py), as above."""
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


def device_ms(fns, reps):
    """medians of `reps` calls of each function after one warm-up each, the functions alternating inside every repetition"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t[i].append(e0.elapsed_time(e1))
    return [float(np.median(x)) for x in t], [float(np.min(x)) for x in t], [float(np.max(x)) for x in t]


def transforms(shape, K, rng):
    c = (np.array(shape) - 1.0) / 2.0
    out = []
    for _ in range(K):
        a = np.deg2rad(rng.uniform(-10.0, 10.0))
        M = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        out.append(np.column_stack([M, c - M @ c + rng.uniform(-3.0, 3.0, 3)]))
    return np.ascontiguousarray(np.stack(out))


def phantom_pair(gn, true_world, voxel):
    """the tests' phantom (field of view 40 x 36 x 32 mm) and its moving image sampled at `voxel` mm"""
    n = lambda mm: int(round(mm / voxel))
    fa = np.diag([voxel, voxel, voxel, 1.0])
    fa[:3, 3] = np.array([-20.0, -18.0, -16.0]) + voxel / 2.0
    ma = np.diag([voxel, voxel, voxel, 1.0])
    ma[:3, 3] = np.array([-22.5, -19.5, -18.5]) + voxel / 2.0
    fixed = gn.phantom_at(gn.grid_world((n(40), n(36), n(32)), fa))
    inv = np.linalg.inv(true_world)
    moving = gn.remap(gn.phantom_at(gn.grid_world((n(44), n(40), n(36)), ma) @ inv[:3, :3].T + inv[:3, 3]))
    return fixed, fa, moving, ma, fixed > 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--voxel", type=float, default=1.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reg-reps", type=int, default=7)
    ap.add_argument("--numpy-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kinds", nargs="+", choices=("mi", "nmi"), default=None, help="measure these mutual-information costs instead (-> profiles/register_mi_bench.json)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "register_mi_bench.json" if a.kinds else "register_bench.json")
    assert torch.cuda.is_available(), "the benchmark needs the device"
    import register_numpy as gn
    reg = importlib.import_module(PKG + ".register")
    rs = importlib.import_module(PKG + ".resample")
    shape = tuple(a.shape)
    rng = np.random.default_rng(0)
    from scipy import ndimage
    fixed = ndimage.gaussian_filter(rng.random(shape), 2.0)
    fixed = (fixed - fixed.min()) / (fixed.max() - fixed.min())
    moving = 1.0 - fixed ** 2
    bins = reg.bin_intensity(fixed, 64)
    dev = torch.device("cuda", 0)
    tf, tm, tb = torch.as_tensor(fixed, device=dev), torch.as_tensor(moving, device=dev), torch.as_tensor(bins, device=dev)
    rows = {"shape": list(shape), "reps": a.reps, "device": torch.cuda.get_device_name(0), "cost_launch": [], "registration": []}
    if a.kinds:
        return main_mi(a, gn, reg, shape, tf, tm, tb, rows)
    for kind in gn.KINDS:
        nb = 64 if kind == "corratio" else 1                       # as register.register calls it
        f = reg.prepare(tf, tb if nb == 64 else torch.zeros_like(tb), tm, kind, nb, 0.25)
        for K in (1, 16, 64):
            A = transforms(shape, K, np.random.default_rng(K))
            (ms, rs_ms), (lo, rs_lo), (hi, rs_hi) = device_ms([lambda: f(A), lambda: rs.resample(tm, A[0], shape, order=1)], a.reps)
            rows["cost_launch"].append({"cost": kind, "n_bins": nb, "K": K, "launch_ms": ms, "launch_ms_min": lo, "launch_ms_max": hi, "ms_per_candidate": ms / K,
                                        "resample_order1_ms": rs_ms, "resample_order1_ms_min": rs_lo, "resample_order1_ms_max": rs_hi,
                                        "candidate_over_resample": ms / K / rs_ms})
            print(json.dumps(rows["cost_launch"][-1]))
    pool = ThreadPoolExecutor(a.threads)

    def threaded(fixed_, bin_, moving_, kind_, n_bins_, min_overlap_):
        def evaluate(A):
            out = list(pool.map(lambda m: gn.cost_one(fixed_, bin_, moving_, m, kind_, n_bins_, min_overlap_, np.float64), A))
            return np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out])
        return evaluate

    for name in ("rigid6", "affine12"):
        p, dof, kind, _ = gn.E2E_CASES[name]
        true_world = reg.params_to_world(p, dof, centre=gn.TRUE_CENTRE)
        fx, fa, mv, ma, mask = phantom_pair(gn, true_world, a.voxel)
        reg.register(fx, fa, mv, ma, dof=6, cost=kind, scales_mm=[8.0], max_sweeps=1)          # warm-up: code objects, allocator
        torch.cuda.synchronize()
        dev_s, host_s = [], []
        for rep in range(max(a.reg_reps, a.numpy_reps)):              # the two legs alternate
            if rep < a.reg_reps:
                t0 = time.perf_counter()
                out = reg.register(fx, fa, mv, ma, dof=dof, cost=kind)
                torch.cuda.synchronize()
                dev_s.append(time.perf_counter() - t0)
            if rep < a.numpy_reps:
                t0 = time.perf_counter()
                ref = reg.register(fx, fa, mv, ma, dof=dof, cost=kind, cost_fn=threaded, filters=gn.FILTERS)
                host_s.append(time.perf_counter() - t0)
        t_dev, t_host = float(np.median(dev_s)), float(np.median(host_s))
        rows["registration"].append({"case": name, "dof": dof, "cost": kind, "fixed_shape": list(fx.shape), "moving_shape": list(mv.shape), "voxel_mm": a.voxel,
                                     "levels_mm": [l["scale_mm"] for l in out["levels"]], "n_eval": sum(l["n_eval"] for l in out["levels"]),
                                     "n_launches": sum(l["n_calls"] for l in out["levels"]), "device_s": t_dev, "device_s_all": dev_s, "numpy_threads": a.threads,
                                     "numpy_s": t_host, "numpy_s_all": host_s, "numpy_n_eval": sum(l["n_eval"] for l in ref["levels"]), "numpy_over_device": t_host / t_dev,
                                     "mean_displacement_mm": gn.mean_displacement(out["world"], true_world, mask, fa),
                                     "numpy_mean_displacement_mm": gn.mean_displacement(ref["world"], true_world, mask, fa)})
        print(json.dumps(rows["registration"][-1]))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


def main_mi(a, gn, reg, shape, tf, tm, tb, rows):
    import register_mi_numpy as mn
    corratio = reg.prepare(tf, tb, tm, "corratio", 64, 0.25)
    for kind in a.kinds:
        f = reg.prepare(tf, tb, tm, kind, 64, 0.25)                # 64 x 64 cells
        for K in (1, 16, 64):
            A = transforms(shape, K, np.random.default_rng(K))
            (ms, cr_ms), (lo, cr_lo), (hi, cr_hi) = device_ms([lambda: f(A), lambda: corratio(A)], a.reps)
            rows["cost_launch"].append({"cost": kind, "n_bins": 64, "moving_bins": 64, "K": K, "launch_ms": ms, "launch_ms_min": lo, "launch_ms_max": hi,
                                        "ms_per_candidate": ms / K, "corratio_ms": cr_ms, "corratio_ms_min": cr_lo, "corratio_ms_max": cr_hi,
                                        "over_corratio": ms / cr_ms})
            print(json.dumps(rows["cost_launch"][-1]))
    pool = ThreadPoolExecutor(a.threads)

    def threaded(fixed_, bin_, moving_, kind_, n_bins_, min_overlap_):
        bin_, moving_ = np.asarray(bin_), np.asarray(moving_, dtype=np.float64)
        mrange = mn.range_of(moving_)

        def one(m):
            y, ins = gn.sample(moving_, m, bin_.shape, np.float64)
            n, n_incl, joint = mn.joint_of_sample(bin_, mrange, y, ins, n_bins_, n_bins_)
            return n, mn.cost_of_joint(joint, kind_, n_incl, min_overlap_, np.float64)

        def evaluate(A):
            out = list(pool.map(one, A))
            return np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out])
        return evaluate

    p, dof, _, _ = gn.E2E_CASES["rigid6"]
    true_world = reg.params_to_world(p, dof, centre=gn.TRUE_CENTRE)
    fx, fa, mv, ma, mask = phantom_pair(gn, true_world, a.voxel)
    for kind in a.kinds:
        reg.register(fx, fa, mv, ma, dof=6, cost=kind, scales_mm=[8.0], max_sweeps=1)          # warm-up: code objects, allocator
        torch.cuda.synchronize()
        dev_s, host_s = [], []
        for rep in range(max(a.reg_reps, a.numpy_reps)):              # the two legs alternate
            if rep < a.reg_reps:
                t0 = time.perf_counter()
                out = reg.register(fx, fa, mv, ma, dof=dof, cost=kind)
                torch.cuda.synchronize()
                dev_s.append(time.perf_counter() - t0)
            if rep < a.numpy_reps:
                t0 = time.perf_counter()
                ref = reg.register(fx, fa, mv, ma, dof=dof, cost=kind, cost_fn=threaded, filters=gn.FILTERS)
                host_s.append(time.perf_counter() - t0)
        t_dev, t_host = float(np.median(dev_s)), float(np.median(host_s))
        rows["registration"].append({"case": "rigid6_" + kind, "dof": dof, "cost": kind, "fixed_shape": list(fx.shape), "moving_shape": list(mv.shape), "voxel_mm": a.voxel,
                                     "levels_mm": [l["scale_mm"] for l in out["levels"]], "n_eval": sum(l["n_eval"] for l in out["levels"]),
                                     "n_launches": sum(l["n_calls"] for l in out["levels"]), "device_s": t_dev, "device_s_all": dev_s, "numpy_threads": a.threads,
                                     "numpy_s": t_host, "numpy_s_all": host_s, "numpy_n_eval": sum(l["n_eval"] for l in ref["levels"]), "numpy_over_device": t_host / t_dev,
                                     "mean_displacement_mm": gn.mean_displacement(out["world"], true_world, mask, fa),
                                     "numpy_mean_displacement_mm": gn.mean_displacement(ref["world"], true_world, mask, fa)})
        print(json.dumps(rows["registration"][-1]))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
