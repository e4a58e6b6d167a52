"""Time of segment='pve' over segment='yes' on a full-size map: the partial-volume stage (met2_partial_volume, motor.partial_volume_filter)
beside the tissue segmentation it follows (met2_tissue_segment) on the same volume in the same process: configs[1]'s geometry, 128 x 128 x 64
voxels of 2 mm, the default parameters of both (3 classes; segmentation: beta 0.1, 4 outer iterations of 8 ICM sweeps after 10 EM steps;
partial volume: beta_pv 0.3, 8 ICM sweeps over 5 types, 64 nodes per mixture).  The volume is the three-class phantom of
tests/tools/bias_numpy.py at that size.  HIP events around each call (the entries are blocking: they allocate and free their work space
inside the call, which the time includes); warm-up calls of both discarded; the two alternate, so that whatever else the machine does
falls on both.  Prints its lines and writes them to --out (default profiles/pve_bench.txt): per filter the median, the best and the worst
time, the launches of a call and the bytes of its work space, and the ratio (segmentation + partial volume) / segmentation, which is what
segment='pve' costs over segment='yes'."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
PKG = "multicomponent-t2-toolbox_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(128, 128, 64))
    ap.add_argument("--voxel", type=float, nargs=3, default=(2.0, 2.0, 2.0))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pve_bench.txt"))
    args = ap.parse_args()
    import bias_numpy as bn
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pve.py needs a GPU: a time taken without one says nothing")
    motor = importlib.import_module(PKG + ".motor")
    dims, vox = tuple(args.dims), tuple(args.voxel)
    v, mask, _, _ = bn.phantom(shape=dims, seed=20261019)
    nvox = int(np.prod(dims))
    K, n_outer, n_em, n_icm = 3, 4, 10, 8
    d = torch.as_tensor(v, device="cuda")
    m = torch.as_tensor(mask, device="cuda")
    seg, prob, _ = motor.tissue_segment_filter(d, m, vox)
    for _ in range(args.warmup):
        motor.tissue_segment_filter(d, m, vox)
        motor.partial_volume_filter(d, None, vox, seg=seg, prob=prob)
    torch.cuda.synchronize()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    ms_seg, ms_pve = [], []
    for _ in range(args.steps):
        t, _ = timed(lambda: motor.tissue_segment_filter(d, m, vox))
        ms_seg.append(t)
        t, (pve, pveseg, mixel, classes) = timed(lambda: motor.partial_volume_filter(d, None, vox, seg=seg, prob=prob))
        ms_pve.append(t)
    t_seg, t_pve = float(np.median(ms_seg)), float(np.median(ms_pve))
    on = mixel != 255
    lines = [
        "segment='pve' over segment='yes': %d x %d x %d voxels of %g x %g x %g mm, %d in the domain, %d steps after %d warm-up calls" % (
            dims + vox + (int(on.sum()), args.steps, args.warmup)),
        "tissue_segment    median %8.3f ms  best %8.3f  worst %8.3f   %4d launches  %10d bytes of work space" % (
            t_seg, min(ms_seg), max(ms_seg), 7 + 2 * n_em + 2 + n_outer * (2 * n_icm + 3) + 2 * n_icm + 2, (22 + 8 * K) * nvox),
        "partial_volume    median %8.3f ms  best %8.3f  worst %8.3f   %4d launches  %10d bytes of work space" % (
            t_pve, min(ms_pve), max(ms_pve), 10 + 2 * n_icm, (8 * (2 * K - 1) + 5) * nvox),
        "(tissue_segment + partial_volume) / tissue_segment = %.3f" % ((t_seg + t_pve) / t_seg),
        "mixed voxels %.1f %% of the domain; class means %s" % (
            100.0 * float((mixel[on] >= K).double().mean()) if int(on.sum()) else 0.0, [round(float(x), 2) for x in classes[:K].cpu()]),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
