#!/usr/bin/env python3
"""Timing of the stages of the non-linear registration (met2_warp, met2_warp_lncc, met2_warp_max_norm2, met2_warp_compose and the two
smoothings) on the device, written to profiles/warp_bench.json:
    python3 scripts/bench_warp.py [--shape 128 128 64] [--radius 2] [--reps 20] [--rounds 2] [--out FILE]
Stages: inputs resident on the device, the median of `reps` calls after a warm-up call, between HIP events on the launch stream; a whole
iteration the same way.  met2_warp order 1 alternates with met2_resample order 1 on the same grid and transform (it reads 24 B per voxel
more); the ratio of the two medians is recorded, not assumed.  The LNCC stage is set against the bytes its algorithm moves through HBM --
per voxel 17 + 48 (first pass: fixed, warped, inside in, six sums out), 96 and 96 (the other two passes), 48 + 17 + 24 (force) = 346 B --
as a share of the 8.0 TB/s peak of the HBM.
Whole registration: the phantom of the tests at 1 mm (40 x 36 x 32) under the tests' field, device stages against the fp64 numpy restatement
(tests/tools/warp_numpy.py, scipy's gaussian_filter; numpy's own threading, the thread count of the run recorded), alternating, `rounds` times
each; host clock around the call, which ends in a copy from the device."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
PKG = "multicomponent-t2-toolbox_amd"
HBM_PEAK = 8.0e12
LNCC_BYTES_PER_VOXEL = (17 + 48) + 96 + 96 + (48 + 17 + 24)


def timed(fns, reps):
    """medians in ms of the callables, alternating between them call by call, after one warm-up call of each"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1))
    return [float(np.median(x)) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 64])
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.json"))
    a = ap.parse_args()
    import register_numpy as gn
    import warp_numpy as wn
    warp = importlib.import_module(PKG + ".warp")
    rs = importlib.import_module(PKG + ".resample")
    shape, r = tuple(a.shape), a.radius
    nvox = int(np.prod(shape))
    rng = np.random.default_rng(0)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    fixed_h = np.clip(0.5 + 0.4 * np.sin(0.11 * i + 0.07 * j) * np.cos(0.13 * k) + 0.02 * rng.standard_normal(shape), 0.0, 1.0)
    fixed, moving = torch.as_tensor(fixed_h, device="cuda"), torch.as_tensor(np.roll(fixed_h, 2, axis=0), device="cuda")
    disp = torch.as_tensor(1.5 * np.stack([np.sin(0.05 * j), np.sin(0.04 * k), np.cos(0.03 * i)], axis=-1), device="cuda").contiguous()
    A = np.ascontiguousarray(np.column_stack([np.eye(3), [0.3, -0.2, 0.1]]))
    S = warp._DeviceStages(0)
    S.begin_level(shape, a.reps)
    state = {}

    def do_warp():
        state["warped"], state["inside"] = S.warp(moving, A, disp)

    def do_resample():
        state["resampled"] = rs.resample(moving, A, shape, order=1, return_inside=True)

    def do_lncc():
        state["force"], state["metric"] = S.lncc(fixed, state["warped"], state["inside"], r, warp.EPS)

    def do_fluid():
        state["v"] = S.smooth(state["force"], 1.5)

    def do_norm():
        state["m2"] = S.max_norm2(state["v"])

    def do_compose():
        state["composed"] = S.compose(disp, shape, warp.IDENTITY, (1.0, 1.0, 1.0), state["v"], 0.25, state["m2"])

    def do_elastic():
        state["next"] = S.smooth(state["composed"], 0.5)

    def iteration():
        for fn in (do_warp, do_lncc, do_fluid, do_norm, do_compose, do_elastic):
            fn()

    iteration()
    warp_ms, resample_ms = timed([do_warp, do_resample], a.reps)
    names = ("lncc", "smooth_fluid", "max_norm2", "compose", "smooth_elastic", "iteration")
    ms = dict(zip(names, timed([do_lncc, do_fluid, do_norm, do_compose, do_elastic, iteration], a.reps)))
    lncc_bytes = LNCC_BYTES_PER_VOXEL * nvox
    rows = {"shape": list(shape), "radius": r, "reps": a.reps, "device": torch.cuda.get_device_name(0),
            "stage_ms": dict(ms, warp_order1=warp_ms, resample_order1=resample_ms), "warp_over_resample": warp_ms / resample_ms,
            "lncc": {"algorithmic_bytes": lncc_bytes, "GBps": lncc_bytes / ms["lncc"] / 1e6, "share_of_hbm_peak": lncc_bytes / (ms["lncc"] * 1e-3) / HBM_PEAK,
                     "hbm_peak_Bps": HBM_PEAK, "valid_voxels": float(state["metric"][1])}}
    print(json.dumps(rows))
    # the whole registration at 1 mm
    aff = np.array([[1.0, 0, 0, -19.5], [0, 1.0, 0, -17.5], [0, 0, 1.0, -15.5], [0, 0, 0, 1.0]])
    P = gn.grid_world((40, 36, 32), aff)
    fx, mv = gn.phantom_at(P), gn.phantom_at(P + wn.true_field(P))
    dev_s, host_s, out_d, out_h = [], [], None, None
    warp.register(fx, aff, mv, aff, None, iters=(1, 1, 1))          # warm-up: code objects, the allocator
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        out_d = warp.register(fx, aff, mv, aff, None, **wn.RECOVERY_OPTIONS)
        dev_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        out_h = warp.register(fx, aff, mv, aff, None, stages=wn.STAGES, filters=gn.FILTERS, **wn.RECOVERY_OPTIONS)
        host_s.append(time.perf_counter() - t0)

    def err(out):
        u = out["disp"] * 1.0                                       # 1 mm voxels
        return float(np.linalg.norm(u + wn.true_field(P + u), axis=-1)[fx > 0.05].mean())

    rows["registration_1mm"] = {"shape": [40, 36, 32], "levels": [list(L["shape"]) for L in out_d["levels"]], "iters": [L["iters"] for L in out_d["levels"]],
                                "device_s": dev_s, "restatement_s": host_s, "restatement_over_device": float(np.median(host_s) / np.median(dev_s)),
                                "host_threads": os.environ.get("OMP_NUM_THREADS", "unset"), "error_before_mm": err({"disp": np.zeros(P.shape)}),
                                "error_after_mm_device": err(out_d), "error_after_mm_restatement": err(out_h),
                                "metric_last_device": out_d["levels"][-1]["metric"][-1], "metric_last_restatement": out_h["levels"][-1]["metric"][-1]}
    print(json.dumps(rows["registration_1mm"]))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
