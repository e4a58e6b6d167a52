#!/usr/bin/env python3
"""Throughput of the label statistics (met2_label_stats) against numpy on the host, measured once per run and appended to
profiles/label_stats_bench.jsonl:
    python3 scripts/bench_label_stats.py [--labels 3 100] [--reps 50] [--threads 16] [--shape 128 128 64] [--out FILE]
The case: a 128 x 128 x 64 volume, 8 maps (series-major) and 60 spectrum bins (voxel-major), every voxel in one of L labels, inputs resident
on the device; the device time is that of the two blocking calls (maps, spectra), the host time numpy's mean / std(ddof=1) / np.quantile
of every (label, series) on `threads` threads.  The bytes the passes move are counted from the algorithm (not from counters): the values
are read three times (two moment passes, one key gather), the member list with every tile of 8 series, the keys written once and read once
per digit level; the algorithmic minimum is one read of the values plus eight key passes."""
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
PKG = "multicomponent-t2-toolbox_amd"


def host_stats(v, members, q, threads):
    """v [S, nvox] -> [L, S, 3 + n_q] with numpy, (label, series) pairs dealt to a thread pool"""
    out = np.empty((len(members), v.shape[0], 3 + len(q)))

    def one(ls):
        l, s = ls
        x = v[s, members[l]]
        x = x[~np.isnan(x)]
        out[l, s, 0] = x.size
        out[l, s, 1] = x.mean()
        out[l, s, 2] = x.std(ddof=1)
        out[l, s, 3:] = np.quantile(x, q)

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, [(l, s) for l in range(len(members)) for s in range(v.shape[0])]))
    return out


def times(fn, reps):
    """-> (median, min, max) seconds of `reps` calls after two warm-up calls; fn blocks until its result is on the host"""
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", type=int, nargs="+", default=[3, 100])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--shape", type=int, nargs=3, default=[128, 128, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_stats_bench.jsonl"))
    a = ap.parse_args()
    importlib.import_module(PKG + "._build").build()
    stats = importlib.import_module(PKG + ".stats")
    rng = np.random.default_rng(0)
    nvox, n_t2 = int(np.prod(a.shape)), 60
    maps = rng.standard_normal((8, nvox))
    maps[0] = np.where(rng.random(nvox) < 0.4, 0.0, 0.1 * np.abs(maps[0]))                  # the MWF's pattern: 40 % exact zeros
    fsol = np.where(rng.random((nvox, n_t2)) < 0.8, 0.0, rng.random((nvox, n_t2)))           # sparse spectra
    q = stats.DEFAULT_Q
    d_maps, d_fsol = torch.as_tensor(maps, device="cuda"), torch.as_tensor(fsol, device="cuda")
    fsol_t = np.ascontiguousarray(fsol.T)
    for L in a.labels:
        lab = rng.integers(0, L, nvox).astype(np.int32)
        d_lab = torch.as_tensor(lab, device="cuda")
        got = [None, None]

        def device():
            got[0] = stats.label_stats(d_maps, d_lab, L, q, "series")
            got[1] = stats.label_stats(d_fsol, d_lab, L, q, "voxel")

        t_dev, t_dev_min, t_dev_max = times(device, a.reps)
        members = [np.nonzero(lab == l)[0] for l in range(L)]
        ref = [None, None]

        def host():
            ref[0] = host_stats(maps, members, q, a.threads)
            ref[1] = host_stats(fsol_t, members, q, a.threads)

        t0 = time.perf_counter()
        host()
        t_host = time.perf_counter() - t0
        same = all(np.array_equal(g[..., 3:], r[..., 3:]) and np.array_equal(g[..., 0], r[..., 0]) for g, r in zip(got, ref))
        S = 8 + n_t2
        big = sum(m.size for m in members if m.size > stats.SMALL_N)
        key_passes = 9 if big else 2                               # written once; read once by the sort in LDS, or once per digit level
        moved = 3 * 8 * nvox * S + 3 * 4 * nvox * ((8 + 7) // 8 + (n_t2 + 7) // 8) + 8 * nvox * S + 8 * big * S * 8 + 8 * (nvox - big) * S
        minimum = 8 * nvox * S + 8 * 8 * nvox * S
        row = {"shape": a.shape, "n_series": S, "n_label": L, "n_q": len(q), "device_s": t_dev, "device_s_min": t_dev_min, "device_s_max": t_dev_max, "reps": a.reps, "host_s": t_host, "host_threads": a.threads,
               "speedup": t_host / t_dev, "quantiles_equal": bool(same), "bytes_moved_model": moved, "bytes_minimum": minimum,
               "moved_over_minimum": moved / minimum, "model_GBps": moved / t_dev / 1e9, "key_passes": key_passes,
               "device": torch.cuda.get_device_name(0), "numpy": np.__version__}
        print(json.dumps(row))
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
