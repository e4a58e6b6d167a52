"""Time of the bias-field correction (met2_bias_field, motor.bias_field_filter) on a full-size map: configs[1]'s geometry, 128 x 128 x 64
voxels of 2 mm, the default parameters (3 classes, 4 outer iterations of 10 EM steps, FWHM 20 mm: radius 17 on every axis).  The volume is
the three-class phantom of tests/tools/bias_numpy.py at that size.  HIP events around each call (the entry is blocking: it allocates and
frees its work space inside the call, which the time includes), one warm-up call discarded.  One JSON line: the median and the best time,
voxels/s, the launches of a call and the bytes of its work space.  --numpy times the numpy restatement on the same volume on the CPU
instead (no GPU needed) and prints its wall time."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
PKG = "multicomponent-t2-toolbox_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(128, 128, 64))
    ap.add_argument("--voxel", type=float, nargs=3, default=(2.0, 2.0, 2.0))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()
    import bias_numpy as bn
    dims, vox = tuple(args.dims), tuple(args.voxel)
    v, mask, _, _ = bn.phantom(shape=dims, seed=20261018)
    nvox = int(np.prod(dims))
    base = {"kernel": "bias_field", "dims": list(dims), "voxel_mm": list(vox), "n_class": 3, "n_outer": 4, "n_em": 10, "fwhm_mm": 20.0,
            "domain_voxels": int((mask != 0).sum())}
    if args.numpy:
        t0 = time.perf_counter()
        bn.bias_field(v, mask, vox)
        base.update({"numpy_restatement_wall_s": round(time.perf_counter() - t0, 3), "cpus": os.cpu_count()})
        print(json.dumps(base))
        return
    import torch
    motor = importlib.import_module(PKG + ".motor")
    d = torch.as_tensor(v, device="cuda")
    m = torch.as_tensor(mask, device="cuda")
    for _ in range(args.warmup):
        motor.bias_field_filter(d, m, vox)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, field, _ = motor.bias_field_filter(d, m, vox, return_field=True)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    t = float(np.median(ms)) * 1e-3
    base.update({"steps": args.steps, "warmup": args.warmup, "ms": round(t * 1e3, 3), "ms_best": round(float(np.min(ms)), 3),
                 "voxels_per_s": round(nvox / t, 1), "launches": 7 + 4 * (2 * 10 + 8) + 1, "work_bytes": 53 * nvox,
                 "field_min": round(float(field.min().item()), 4), "field_max": round(float(field.max().item()), 4)})
    print(json.dumps(base))


if __name__ == "__main__":
    main()
