"""Throughput of the bootstrap mode (met2_fit_bootstrap): replicate fits per second for 65 536 voxels x B = 100 at configs[1]'s shape
(32 x 60, X2/L2) and at 48 x 120 (GCV/L2), beside the plain fit's voxels/s on the same plan.  One JSON line per configuration.
The kernels' shares of the GPU time come from a run under rocprofv3:
    rocprofv3 --kernel-trace --stats -d DIR -o s --output-format csv -- python scripts/bench_bootstrap.py --steps 1
    python scripts/bench_bootstrap.py --shares DIR/s_kernel_stats.csv        # one JSON line, no GPU needed"""
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

CONFIGS = [("X2", "L2", 32, 60), ("GCV", "L2", 48, 120)]


def shares(path):
    """GPU-time shares of the bootstrap's own kernels and of the fit kernels in a rocprofv3 kernel_stats CSV."""
    import csv
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    part = lambda key: sum(float(r["TotalDurationNs"]) for r in rows if key in r["Name"]) / total
    print(json.dumps({"kernel_stats": os.path.basename(path), "gpu_ms": round(total / 1e6, 1),
                      "share_bootstrap_gen_kernel": round(part("bootstrap_gen_kernel"), 5),
                      "share_bootstrap_stats_kernel": round(part("bootstrap_stats_kernel"), 5),
                      "share_bootstrap_sigma_kernel": round(part("bootstrap_sigma_kernel"), 5), "share_fit_kernels": round(part("fit_kernel<"), 5)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=65536)
    ap.add_argument("--n-rep", type=int, default=100)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--shares", metavar="KERNEL_STATS_CSV", help="only summarise a rocprofv3 kernel_stats CSV of a run of this script")
    args = ap.parse_args()
    if args.shares:
        return shares(args.shares)
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    for method, pen, nte, nt2 in CONFIGS:
        T2s = synth.t2_grid(nt2)
        plan = pkg.Met2Plan(nte, nt2, 1, device=0)
        plan.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, np.array([150.0]), 3000.0).set_penalty(pen, T2s)
        data, _, _ = synth.make_voxels(args.voxels, nte=nte, seed=20261016, device="cuda:0")
        point_in, _, _ = synth.make_voxels(262144, nte=nte, seed=20261017, device="cuda:0")
        plan.fit(method, point_in)                                     # warm-up: scratch, code objects
        torch.cuda.synchronize()
        t = time.perf_counter()
        plan.fit(method, point_in)
        torch.cuda.synchronize()
        point_vps = point_in.shape[0] / (time.perf_counter() - t)
        plan.fit_bootstrap(method, data[:4096].contiguous(), n_rep=args.n_rep, seed=1)       # warm-up: the bootstrap's scratch
        walls = []
        for s in range(args.steps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = plan.fit_bootstrap(method, data, n_rep=args.n_rep, seed=s)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t)
        wall = min(walls)
        rows = args.voxels * args.n_rep
        print(json.dumps({"config": "%s/%s %dx%d" % (method, pen, nte, nt2), "voxels": args.voxels, "n_rep": args.n_rep,
                          "wall_s": round(wall, 4), "replicate_fits_per_s": round(rows / wall), "point_fit_voxels_per_s": round(point_vps),
                          "replicate_over_point": round(rows / wall / point_vps, 3),
                          "fitted_voxels": int(((out["status"] & 1) != 0).sum().item())}), flush=True)
        plan.close()


if __name__ == "__main__":
    main()
