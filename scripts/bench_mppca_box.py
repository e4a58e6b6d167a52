"""Times of the MP-PCA denoiser with a box window and overlapping-patch averaging (met2_mppca_box, filters.mppca_filter) beside met2_mppca,
on the volume of scripts/bench_mppca.py: 128 x 128 x 64 voxels of 32 echoes, every voxel inside the mask.  Per window: met2_mppca (cubic
windows only), met2_mppca_box with average = 0 and with average = 1.  The variants are run in turn, round after round and every other round in reverse order, so that
a drift of the machine touches them alike; a host clock around each call, which ends in a device synchronise; the warm-up rounds are discarded; the
median, the best and the worst of the rounds are reported, in ms and in ms per Mi voxels.  The cubic average = 0 result is compared with
met2_mppca's bit for bit.  --only <variant> runs one variant alone (for a kernel trace: the share of the averaging kernel is the trace's)."""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
PKG = "multicomponent-t2-toolbox_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(128, 128, 64))
    ap.add_argument("--nt", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bench_mppca import volume
    filters = importlib.import_module(PKG + ".filters")
    dims = tuple(args.dims)
    d = volume(dims, args.nt, 10.0, 20260113)
    m = torch.ones(dims, dtype=torch.uint8, device=d.device)
    variants = {"met2_mppca w=5": dict(window=5), "box (5,5,5) average=0": dict(window=(5, 5, 5)), "box (5,5,5) average=1": dict(window=(5, 5, 5), average=True),
                "box (5,5,1) average=0": dict(window=(5, 5, 1)), "box (5,5,1) average=1": dict(window=(5, 5, 1), average=True)}
    if args.only:
        variants = {args.only: variants[args.only]}
    ms = {k: [] for k in variants}
    kept = {}
    for it in range(args.warmup + args.steps):
        for name, kw in (list(variants.items())[::-1] if it % 2 else variants.items()):   # every other round in reverse order
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = filters.mppca_filter(d, m, return_maps=True, **kw)
            torch.cuda.synchronize()
            if it >= args.warmup:
                ms[name].append(1e3 * (time.perf_counter() - t0))
            kept[name] = res
    mi = float(np.prod(dims)) / 2 ** 20
    lines = ["MP-PCA, %d x %d x %d voxels of %d echoes, %d rounds after %d warm-up: ms per call (median / best / worst), ms per Mi voxels (median)"
             % (dims + (args.nt, args.steps, args.warmup))]
    for name, t in ms.items():
        out, sigma, rank = kept[name]
        rk = torch.bincount(rank.reshape(-1).clamp(min=0), minlength=4).double() / rank.numel()
        lines.append("%-24s %9.2f / %9.2f / %9.2f   %9.2f   mean rank %.2f, median sigma %.3f" % (
            name, np.median(t), min(t), max(t), np.median(t) / mi, float((rk * torch.arange(rk.numel(), device=rk.device)).sum()), float(sigma.median())))
    if "met2_mppca w=5" in kept and "box (5,5,5) average=0" in kept:
        eq = all(torch.equal(a, b) for a, b in zip(kept["met2_mppca w=5"], kept["box (5,5,5) average=0"]))
        lines.append("box (5,5,5) average=0 equals met2_mppca w=5 bit for bit: %s" % eq)
    for w in ((5, 5, 5), (5, 5, 1)):
        lines.append("work space %s: min %d bytes, default %d bytes" % ((w,) + filters.mppca_work_bytes(dims + (args.nt,), w)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
