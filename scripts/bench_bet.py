"""Time of the brain extraction (met2_brain_mask, motor.brain_mask_filter) on a full-size echo mean: configs[1]'s geometry, 128 x 128 x 64
voxels of 2 mm, the default parameters (f = 0.4, level 4 = 2562 vertices, 1000 iterations).  The volume is the nested-ellipsoid phantom of
tests/tools/bet_numpy.py at that size.  HIP events around each call (the entries are blocking: they allocate and free their work space
inside the call, which the time includes), one warm-up call discarded, the median of --steps calls: the whole filter, and the stages through
their own entries (statistics; evolution at n_iter and at 0 iterations, whose difference over n_iter is the evolution kernel's time per
iteration; fill).  One JSON line.  --numpy times the numpy restatement on the same volume on the CPU instead (no GPU needed)."""
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
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--n-iter", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()
    import bet_numpy as bn
    dims, vox = tuple(args.dims), tuple(args.voxel)
    v, lab = bn.phantom(dims, vox, seed=20261018)
    brain = lab == 1
    dice = lambda m: round(float(2.0 * (m.astype(bool) & brain).sum() / (m.sum() + brain.sum())), 4)
    base = {"kernel": "brain_mask", "dims": list(dims), "voxel_mm": list(vox), "f": 0.4, "level": args.level, "n_iter": args.n_iter,
            "vertices": 10 * 4 ** args.level + 2}
    if args.numpy:
        t0 = time.perf_counter()
        st = bn.stats(v, vox)
        t1 = time.perf_counter()
        X = bn.evolve(v, vox, st, bn.start_vertices(st, args.level), args.level, 0.4, args.n_iter)
        t2 = time.perf_counter()
        mask = bn.fill(X, bn.icosphere(args.level)[1], dims, vox)
        t3 = time.perf_counter()
        base.update({"numpy_restatement_wall_s": round(t3 - t0, 3), "numpy_stats_s": round(t1 - t0, 3), "numpy_evolve_s": round(t2 - t1, 3),
                     "numpy_fill_s": round(t3 - t2, 3), "dice_vs_true_brain": dice(mask), "cpus": os.cpu_count()})
        print(json.dumps(base))
        return
    import torch
    motor = importlib.import_module(PKG + ".motor")
    bet = importlib.import_module(PKG + ".bet")
    d = torch.as_tensor(v, device="cuda")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), out

    kw = {"f": 0.4, "level": args.level, "n_iter": args.n_iter}
    total, total_best, (mask, verts, tris, st) = timed(lambda: motor.brain_mask_filter(d, vox, return_surface=True, **kw))
    s_ms, _, st2 = timed(lambda: bet.bet_stats(d, vox))
    x0 = torch.as_tensor(bn.start_vertices(st, args.level), device="cuda")
    e_ms, _, _ = timed(lambda: bet.bet_evolve(d, vox, st, x0, args.level, 0.4, args.n_iter))
    e0_ms, _, _ = timed(lambda: bet.bet_evolve(d, vox, st, x0, args.level, 0.4, 0))
    t_dev = torch.as_tensor(tris, device="cuda")
    f_ms, _, _ = timed(lambda: bet.bet_fill(verts, t_dev, dims, vox))
    base.update({"steps": args.steps, "warmup": args.warmup, "ms": round(total, 3), "ms_best": round(total_best, 3), "stats_ms": round(s_ms, 3),
                 "evolve_ms": round(e_ms, 3), "evolve_0_iterations_ms": round(e0_ms, 3),
                 "evolve_us_per_iteration": round((e_ms - e0_ms) * 1e3 / max(args.n_iter, 1), 3), "fill_ms": round(f_ms, 3),
                 "evolve_lds_bytes": 60 * (10 * 4 ** args.level + 2), "mask_voxels": int(mask.sum().item()),
                 "dice_vs_true_brain": dice(mask.cpu().numpy()), "stats": {k: round(x, 4) for k, x in st.items()}})
    print(json.dumps(base))


if __name__ == "__main__":
    main()
