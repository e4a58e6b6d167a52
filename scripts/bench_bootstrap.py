"""Throughput of the bootstrap mode (met2_fit_bootstrap): replicate fits per second for 65 536 voxels x B = 100 at configs[1]'s shape
(32 x 60, X2/L2) and at 48 x 120 (GCV/L2), beside the plain fit's voxels/s on the same plan.  One JSON line per configuration.
--fa brute-force | spline re-estimates the flip angle of every replicate (met2_fit_bootstrap_fa) on a plan with the driver's FA axis (91 angles
from 90 to 180 degrees; 273 and a 15-angle coarse plan for the spline method), the voxels' true angles drawn from that grid; --spectrum also
takes the per-bin statistics of the replicates' spectra.  Without either the run is the parent's: one flip angle, met2_fit_bootstrap.
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
                      "share_bootstrap_spec_stats_kernel": round(part("bootstrap_spec_stats_kernel"), 5),
                      "share_fa_project_and_walk": round(part("fa_project_kernel") + part("fa_kernel<") + part("fa_spline_kernel"), 5),
                      "share_bootstrap_sigma_kernel": round(part("bootstrap_sigma_kernel"), 5), "share_fit_kernels": round(part("fit_kernel<"), 5)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=65536)
    ap.add_argument("--n-rep", type=int, default=100)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--fa", choices=("fixed", "brute-force", "spline"), default="fixed")
    ap.add_argument("--spectrum", action="store_true")
    ap.add_argument("--config", type=int, choices=(0, 1), help="only this entry of CONFIGS")
    ap.add_argument("--shares", metavar="KERNEL_STATS_CSV", help="only summarise a rocprofv3 kernel_stats CSV of a run of this script")
    args = ap.parse_args()
    if args.shares:
        return shares(args.shares)
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    kw = {} if args.fa == "fixed" and not args.spectrum else {"fa": args.fa, "want_spectrum": args.spectrum}
    for method, pen, nte, nt2 in (CONFIGS if args.config is None else CONFIGS[args.config:args.config + 1]):
        T2s = synth.t2_grid(nt2)
        alphas = np.array([150.0]) if args.fa == "fixed" else np.linspace(90.0, 180.0, 273 if args.fa == "spline" else 91)
        plan = pkg.Met2Plan(nte, nt2, alphas.shape[0], device=0)
        plan.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, alphas, 3000.0).set_penalty(pen, T2s)
        coarse = None
        if args.fa == "spline":
            coarse = pkg.Met2Plan(nte, nt2, 15, device=0)
            coarse.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, np.linspace(90.0, 180.0, 15), 3000.0)
            plan.attach_fa_spline(coarse, np.linspace(90.0, 180.0, 15))
        grid = None if args.fa == "fixed" else alphas
        data, fa_true, _ = synth.make_voxels(args.voxels, nte=nte, seed=20261016, fa_values=grid, device="cuda:0")
        point_in, point_fa, _ = synth.make_voxels(262144, nte=nte, seed=20261017, fa_values=grid, device="cuda:0")
        if fa_true is not None:
            kw["fa_index"] = fa_true
        plan.fit(method, point_in, fa_index=point_fa)                  # warm-up: scratch, code objects
        torch.cuda.synchronize()
        t = time.perf_counter()
        plan.fit(method, point_in, fa_index=point_fa)
        torch.cuda.synchronize()
        point_vps = point_in.shape[0] / (time.perf_counter() - t)
        wkw = dict(kw, fa_index=kw["fa_index"][:4096]) if "fa_index" in kw else kw
        plan.fit_bootstrap(method, data[:4096].contiguous(), n_rep=args.n_rep, seed=1, **wkw)       # warm-up: the bootstrap's scratch
        walls = []
        for s in range(args.steps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = plan.fit_bootstrap(method, data, n_rep=args.n_rep, seed=s, **kw)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t)
        wall = min(walls)
        rows = args.voxels * args.n_rep
        print(json.dumps({"config": "%s/%s %dx%d" % (method, pen, nte, nt2), "fa": args.fa, "spectrum": args.spectrum, "n_fa": int(alphas.shape[0]),
                          "voxels": args.voxels, "n_rep": args.n_rep, "walls_s": [round(x, 4) for x in walls],
                          "wall_s": round(wall, 4), "replicate_fits_per_s": round(rows / wall), "point_fit_voxels_per_s": round(point_vps),
                          "replicate_over_point": round(rows / wall / point_vps, 3),
                          "fitted_voxels": int(((out["status"] & 1) != 0).sum().item())}), flush=True)
        plan.close()
        if coarse is not None:
            coarse.close()


if __name__ == "__main__":
    main()
