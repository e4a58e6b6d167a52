"""Time of the tissue segmentation (met2_tissue_segment, motor.tissue_segment_filter) on a full-size map, beside the bias-field correction
(met2_bias_field) on the same volume in the same process: configs[1]'s geometry, 128 x 128 x 64 voxels of 2 mm, the default parameters of
both (3 classes; segmentation: beta 0.1, 4 outer iterations of 8 ICM sweeps after 10 EM steps; bias: 4 outer iterations of 10 EM steps,
FWHM 20 mm).  The volume is the three-class phantom of tests/tools/bias_numpy.py at that size.  HIP events around each call (the entries are
blocking: they allocate and free their work space inside the call, which the time includes); warm-up calls of both discarded; the two
alternate, so that whatever else the machine does falls on both.  One JSON line, also written to --out (default
profiles/segment_bench.json): per filter the median, the best and the spread of the times, voxels/s, the launches of a call and the bytes of
its work space.  The step is bound by its launches (n_outer (2 n_icm + 3) + ...), not by bandwidth: no bandwidth figure is derived."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
PKG = "multicomponent-t2-toolbox_amd"


def summary(ms, nvox):
    t = float(np.median(ms))
    return {"ms": round(t, 3), "ms_best": round(float(np.min(ms)), 3), "ms_worst": round(float(np.max(ms)), 3),
            "voxels_per_s": round(nvox / (t * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(128, 128, 64))
    ap.add_argument("--voxel", type=float, nargs=3, default=(2.0, 2.0, 2.0))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_bench.json"))
    args = ap.parse_args()
    import bias_numpy as bn
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment.py needs a GPU: a time taken without one says nothing")
    motor = importlib.import_module(PKG + ".motor")
    dims, vox = tuple(args.dims), tuple(args.voxel)
    v, mask, _, _ = bn.phantom(shape=dims, seed=20261019)
    nvox = int(np.prod(dims))
    K, n_outer, n_em, n_icm = 3, 4, 10, 8
    d = torch.as_tensor(v, device="cuda")
    m = torch.as_tensor(mask, device="cuda")
    for _ in range(args.warmup):
        motor.tissue_segment_filter(d, m, vox)
        motor.bias_field_filter(d, m, vox, return_field=True)
    torch.cuda.synchronize()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    ms_seg, ms_bias = [], []
    for _ in range(args.steps):
        t, (seg, prob, classes) = timed(lambda: motor.tissue_segment_filter(d, m, vox))
        ms_seg.append(t)
        t, _ = timed(lambda: motor.bias_field_filter(d, m, vox, return_field=True))
        ms_bias.append(t)
    res = {"kernel": "tissue_segment", "dims": list(dims), "voxel_mm": list(vox), "n_class": K, "beta": 0.1, "n_outer": n_outer, "n_em": n_em,
           "n_icm": n_icm, "domain_voxels": int((mask != 0).sum()), "steps": args.steps, "warmup": args.warmup,
           "segment": dict(summary(ms_seg, nvox), launches=7 + 2 * n_em + 2 + n_outer * (2 * n_icm + 3) + 2 * n_icm + 2,
                           work_bytes=(22 + 8 * K) * nvox),
           "bias_field": dict(summary(ms_bias, nvox), launches=7 + 4 * (2 * 10 + 8) + 1, work_bytes=53 * nvox),
           "labels_in_use": int(len(torch.unique(seg[seg > 0]))), "class_means": [round(float(x), 4) for x in classes[:K].cpu()]}
    res["segment_over_bias"] = round(res["segment"]["ms"] / res["bias_field"]["ms"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
