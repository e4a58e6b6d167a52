#!/usr/bin/env python3
"""Timing of the affine resampling (met2_resample) on the device, against a device-to-device copy of the same bytes and against
scipy.ndimage.affine_transform on the host, written to profiles/resample_bench.json:
    python3 scripts/bench_resample.py [--shape 128 128 64] [--series 8] [--reps 5] [--threads 16] [--out FILE]
The case: `series` volumes of 128 x 128 x 64 onto a grid of the same size under a 10 degree rotation about z with a scaling of 1.05 about the
centre, inputs resident on the device, series-major ([S, x, y, z]) and voxel-major ([x, y, z, S]); orders 0, 1 and 3, and the prefilter of
order 3 alone.  Device times are the median of `reps` calls after one warm-up call, between HIP events on the launch stream (an order-3 call
allocates and frees its work space and waits for the device: that is inside its time).  The host leg deals (series, slab of the output)
pairs to `threads` threads, the prefilter of order 3 once per series; its single-thread time is given beside it."""
import argparse
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multicomponent-t2-toolbox_amd"


def transform(shape):
    a = np.deg2rad(10.0)
    M = 1.05 * np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = (np.array(shape) - 1.0) / 2.0
    return np.ascontiguousarray(np.column_stack([M, c - M @ c]))


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t))


def host_s(v, A, order, threads):
    """scipy on `threads` threads: the output of every series cut into slabs along x"""
    S, shape = v.shape[0], v.shape[1:]
    out = np.empty_like(v)
    n_slab = max(1, threads // S) if threads > 1 else 1
    edges = np.linspace(0, shape[0], n_slab + 1).astype(int)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        coef = list(pool.map(lambda s: ndimage.spline_filter(v[s], order=3, mode="mirror"), range(S))) if order == 3 else v

        def one(job):
            s, k = job
            x0, x1 = edges[k], edges[k + 1]
            out[s, x0:x1] = ndimage.affine_transform(coef[s], A[:, :3], offset=A[:, 3] + A[:, 0] * x0, output_shape=(x1 - x0,) + shape[1:], order=order,
                                                     mode="constant", cval=0.0, prefilter=False)

        list(pool.map(one, [(s, k) for s in range(S) for k in range(n_slab)]))
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 64])
    ap.add_argument("--series", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    rs = importlib.import_module(PKG + ".resample")
    shape, S = tuple(a.shape), a.series
    rng = np.random.default_rng(0)
    v = rng.standard_normal((S,) + shape)
    A = transform(shape)
    nbytes = v.nbytes
    src = {"series": torch.as_tensor(v, device="cuda"), "voxel": torch.as_tensor(np.ascontiguousarray(np.moveaxis(v, 0, -1)), device="cuda")}
    dst = torch.empty_like(src["series"])
    copy_ms = device_ms(lambda: dst.copy_(src["series"]), a.reps)
    rows = {"shape": list(shape), "n_series": S, "bytes_in": nbytes, "reps": a.reps, "copy_ms": copy_ms, "copy_GBps": 2 * nbytes / copy_ms / 1e6,
            "device": torch.cuda.get_device_name(0), "host_threads": a.threads, "scipy": importlib.import_module("scipy").__version__, "cases": []}
    for order in (0, 1, 3):
        t_host, ref = host_s(v, A, order, a.threads)
        t_host1 = host_s(v[:1], A, order, 1)[0] * S
        for layout in ("series", "voxel"):
            got = [None]

            def call():
                got[0] = rs.resample(src[layout], A, shape, order=order, layout=layout)

            ms = device_ms(call, a.reps)
            out = got[0].cpu().numpy()
            out = out if layout == "series" else np.moveaxis(out, -1, 0)
            rows["cases"].append({"what": "order %d" % order, "layout": layout, "device_ms": ms, "over_copy": ms / copy_ms, "scipy_s": t_host,
                                  "scipy_one_thread_s": t_host1, "scipy_over_device": t_host / (ms / 1e3),
                                  "max_abs_diff_to_scipy": float(np.abs(out - ref).max())})
            print(json.dumps(rows["cases"][-1]))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as pool:
        ref = np.stack(list(pool.map(lambda s: ndimage.spline_filter(v[s], order=3, mode="mirror"), range(S))))
    t_host = time.perf_counter() - t0
    for layout in ("series", "voxel"):
        got = [None]

        def call():
            got[0] = rs.prefilter(src[layout], layout=layout)

        ms = device_ms(call, a.reps)
        rows["cases"].append({"what": "prefilter", "layout": layout, "device_ms": ms, "over_copy": ms / copy_ms, "scipy_s": t_host,
                              "scipy_over_device": t_host / (ms / 1e3), "max_abs_diff_to_scipy": float(np.abs(got[0].cpu().numpy() - ref).max())})
        print(json.dumps(rows["cases"][-1]))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
