#!/usr/bin/env python3
"""Timing of the inverse of a displacement field (met2_warp_invert_step, met2_warp_jacobian, warp.invert) on the device, written to
profiles/warp_inverse_bench.json:
    python3 scripts/bench_warp_inverse.py [--shape 128 128 64] [--reps 20] [--out FILE]
Kernels: inputs resident on the device, outputs allocated before, the median of `reps` calls after a warm-up call, between HIP events on the
launch stream.  One invert_step (v_in given, inside and res2 asked for) alternates call by call with one met2_warp_compose on the same grid,
transform and fields (v given, the device scalar given): the step does compose's memory work plus a 3 x 3 product, the inside byte and a
block maximum; the ratio of the two medians is recorded, not assumed.  Bytes per voxel by the algorithm: the step reads v_in (24) and writes
v_out (24) and inside (1), and gathers 8 taps of 24 B from u_src, of which neighbouring voxels share all but one voxel's worth -- 24 B where
the gather is served once, so 73 B; compose the same without the inside byte, 72 B; the Jacobian reads the field once (24; its six neighbours
are other voxels' own reads) and writes 8, so 32 B.  They are set against the 8.0 TB/s peak of the HBM -- with the caveat of DESIGN.md 17b:
at 128 x 128 x 64 a field is 25 MB, all of them fit the 256 MB Infinity Cache, so a share above what HBM could give is the cache's doing.
The step is also timed without `inside` and res2, with either alone, and next to a one-element fill on the stream (what zeroing *res2 costs
as a launch of its own), to say where the time above compose goes.
The loop: a 20-step warp.invert on that grid and on a small one, alternating call by call with the same call with 0 steps (host clock
around the call, which begins with a copy to the device and ends with one from it; medians of `reps`): the difference over 20 is the cost
of a step in the loop, on the small grid the launch cost per step."""
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
PKG = "multicomponent-t2-toolbox_amd"
HBM_PEAK = 8.0e12
BYTES_PER_VOXEL = {"invert_step": 24 + 24 + 1 + 24, "compose": 24 + 24 + 24, "jacobian": 24 + 8}


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


def field(shape):
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.ascontiguousarray(1.5 * np.stack([np.sin(0.05 * j) * np.cos(0.04 * k), np.sin(0.04 * k), np.cos(0.03 * i) * np.sin(0.05 * j)], axis=-1))


def loop_seconds(warp, u, A, shape, counts, rounds):
    """medians in s of warp.invert with each of the step counts, alternating between them call by call, after a warm-up call of each"""
    for n in counts:
        warp.invert(u, A, shape, n_iter=n)
    t = [[] for _ in counts]
    for _ in range(rounds):
        for k, n in enumerate(counts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            warp.invert(u, A, shape, n_iter=n)
            t[k].append(time.perf_counter() - t0)
    return [float(np.median(x)) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 64])
    ap.add_argument("--small", type=int, nargs=3, default=[20, 18, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_inverse_bench.json"))
    a = ap.parse_args()
    warp = importlib.import_module(PKG + ".warp")
    rs = importlib.import_module(PKG + ".resample")
    L = importlib.import_module(PKG + "._lib").lib()
    dp = importlib.import_module(PKG + "._lib")._dp
    shape = tuple(a.shape)
    nvox = int(np.prod(shape))
    A = np.ascontiguousarray(np.column_stack([np.diag([1.02, 0.98, 1.0]), [0.3, -0.2, 0.1]]))
    B = np.ascontiguousarray(rs.invert(A)[:3])
    N = np.ascontiguousarray(-A[:, :3])
    gain = np.ones(3)
    dev = torch.device("cuda", 0)
    u_h = field(shape)
    u = torch.as_tensor(u_h, device=dev)
    v_in = torch.as_tensor(0.5 * u_h[..., ::-1].copy(), device=dev)
    v_out, composed = torch.empty_like(u), torch.empty_like(u)
    inside = torch.empty(shape, dtype=torch.uint8, device=dev)
    res2, m2 = torch.zeros(1, dtype=torch.float64, device=dev), torch.ones(1, dtype=torch.float64, device=dev)
    det = torch.empty(shape, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    i3, st = rs._i3(shape), rs._stream(dev)

    def do_step():
        warp._step_into(dev, shape, u, shape, B, N, v_in, v_out, inside, res2)

    def do_step_bare():
        warp._step_into(dev, shape, u, shape, B, N, v_in, v_out, None, None)

    def do_step_inside():
        warp._step_into(dev, shape, u, shape, B, N, v_in, v_out, inside, None)

    def do_step_res2():
        warp._step_into(dev, shape, u, shape, B, N, v_in, v_out, None, res2)

    def do_zero():
        res2.zero_()                                               # a fill of one element on the stream: what zeroing *res2 costs as a launch of its own

    def do_compose():
        warp.check(L.met2_warp_compose(0, i3, u.data_ptr(), i3, B.ctypes.data_as(dp), gain.ctypes.data_as(dp), v_in.data_ptr(), 1.0, m2.data_ptr(),
                                       composed.data_ptr(), st))

    def do_jacobian():
        warp.check(L.met2_warp_jacobian(0, i3, u.data_ptr(), 1.0, det.data_ptr(), count.data_ptr(), st))

    step_ms, compose_ms = timed([do_step, do_compose], a.reps)
    bare_ms, inside_ms, res2_ms, zero_ms, jac_ms = timed([do_step_bare, do_step_inside, do_step_res2, do_zero, do_jacobian], a.reps)
    ms = {"invert_step": step_ms, "compose": compose_ms, "invert_step_no_inside_no_res2": bare_ms, "invert_step_inside_only": inside_ms,
          "invert_step_res2_only": res2_ms, "fill_one_element": zero_ms, "jacobian": jac_ms}
    rows = {"shape": list(shape), "reps": a.reps, "device": torch.cuda.get_device_name(0), "kernel_ms": ms, "invert_step_over_compose": step_ms / compose_ms,
            "hbm_peak_Bps": HBM_PEAK, "fits_infinity_cache": bool(3 * 24 * nvox < 256 * 2 ** 20),
            "algorithmic": {k: {"bytes_per_voxel": b, "GBps": b * nvox / ms[k] / 1e6, "share_of_hbm_peak": b * nvox / (ms[k] * 1e-3) / HBM_PEAK}
                            for k, b in BYTES_PER_VOXEL.items()}}
    print(json.dumps(rows))
    loops = {}
    for name, shp in (("large", shape), ("small", tuple(a.small))):
        uh = field(shp)
        s0, s20 = loop_seconds(warp, uh, A, shp, (0, 20), a.reps)
        loops[name] = {"shape": list(shp), "invert_0_steps_ms": 1e3 * s0, "invert_20_steps_ms": 1e3 * s20, "per_step_ms": 1e3 * (s20 - s0) / 20.0}
    rows["loop"] = loops
    print(json.dumps(loops))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
