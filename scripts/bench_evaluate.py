"""Throughput of the Monte-Carlo accuracy study (met2_amd.evaluate.evaluate_methods): voxel-fits per second (voxels x 10 methods / wall
time, generation, flip-angle search, fits, metrics and reduction included) for one SNR band of 10 000 and of 1 000 000 voxels at the
study's shape (32 x 60, 91 flip angles).  One JSON line per size.  The kernels' shares of the GPU time come from a run under rocprofv3:
    rocprofv3 --kernel-trace --stats -d DIR -o s --output-format csv -- python scripts/bench_evaluate.py --steps 1
    python scripts/bench_evaluate.py --shares DIR/s_kernel_stats.csv        # one JSON line, no GPU needed"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multicomponent-t2-toolbox_amd"


def shares(path):
    """GPU-time shares of the study's own kernels and of the fit kernels in a rocprofv3 kernel_stats CSV."""
    import csv
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    part = lambda key: sum(float(r["TotalDurationNs"]) for r in rows if key in r["Name"]) / total
    print(json.dumps({"kernel_stats": os.path.basename(path), "gpu_ms": round(total / 1e6, 1),
                      "share_synth_two_lobe_kernel": round(part("synth_two_lobe_kernel"), 5),
                      "share_eval_voxel_metrics_kernel": round(part("eval_voxel_metrics_kernel"), 5),
                      "share_eval_reduce_kernel": round(part("eval_reduce_kernel"), 5), "share_fit_kernels": round(part("fit_kernel<"), 5)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 1000000])
    ap.add_argument("--snr", type=float, nargs=2, default=[50.0, 150.0])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--shares", metavar="KERNEL_STATS_CSV", help="only summarise a rocprofv3 kernel_stats CSV of a run of this script")
    args = ap.parse_args()
    if args.shares:
        return shares(args.shares)
    ev = importlib.import_module(PKG + ".evaluate")
    ev.evaluate_methods(n_voxels=4096, snr=tuple(args.snr), seed=99)                # warm-up: code objects, plan scratch
    for n in args.sizes:
        walls = []
        for s in range(args.steps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = ev.evaluate_methods(n_voxels=n, snr=tuple(args.snr), seed=s)
            walls.append(time.perf_counter() - t)
        wall = min(walls)
        nm = len(res.methods)
        print(json.dumps({"voxels": n, "snr": args.snr, "methods": nm, "shape": "32x60x91", "wall_s": round(wall, 4),
                          "voxel_fits_per_s": round(n * nm / wall), "voxels_per_s": round(n / wall),
                          "mae_mwf_x2_l2": round(float(res.errors[3, 0]), 6)}), flush=True)


if __name__ == "__main__":
    main()
