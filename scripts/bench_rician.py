"""Times of the Rician noise-floor correction on configs[1]'s geometry (128 x 128 x 64 voxels of 32 echoes as [nvox, n_te] rows): the kernels
met2_rician_step and met2_rician_invert against a device-to-device copy with the same memory traffic in the same process (both kernels are
elementwise: 24 B per sample -- data and model in, out back for step; the copy moves 12 B per sample in and 12 B out), and
Met2Plan.fit_rician(n_iter=3) against Met2Plan.fit (X2 / L2, 91 flip angles, FA index given) on the same volume.  The volume is a two-pool
decay with spatial gradients, peak 1000, Rician noise of sigma 10.  HIP events around each call, the median of the calls after the warm-up.
One JSON line, also written to --out."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multicomponent-t2-toolbox_amd"


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(128, 128, 64))
    ap.add_argument("--nt", type=int, default=32)
    ap.add_argument("--noise", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fit-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    rician = importlib.import_module(PKG + ".rician")
    dev = torch.device("cuda", 0)
    nvox, nt = int(np.prod(a.dims)), a.nt
    g = torch.Generator(device=dev).manual_seed(20260114)
    u = torch.rand((3, nvox, 1), dtype=torch.float64, device=dev, generator=g)
    te = 10.0 * torch.arange(1, nt + 1, dtype=torch.float64, device=dev)
    f = 0.1 + 0.15 * u[0]
    s = 1000.0 * (f * torch.exp(-te / (15.0 + 10.0 * u[1])) + (1.0 - f) * torch.exp(-te / (70.0 + 30.0 * u[2])))
    re = s + a.noise * torch.randn(s.shape, dtype=torch.float64, device=dev, generator=g)
    im = a.noise * torch.randn(s.shape, dtype=torch.float64, device=dev, generator=g)
    data = torch.sqrt(re * re + im * im)
    sigma = torch.full((nvox,), a.noise, dtype=torch.float64, device=dev)
    del re, im, u
    src = torch.empty((nvox * nt * 3) // 2, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    res = {"kernel": "rician", "dims": list(a.dims), "nt": nt, "noise": a.noise, "steps": a.steps, "warmup": a.warmup}
    res["copy_ms"] = round(timed(lambda: dst.copy_(src), a.steps, a.warmup), 4)
    res["step_ms"] = round(timed(lambda: rician.step(data, s, sigma), a.steps, a.warmup), 4)
    res["invert_ms"] = round(timed(lambda: rician.invert(data, sigma), a.steps, a.warmup), 4)
    res["step_over_copy"] = round(res["step_ms"] / res["copy_ms"], 3)
    res["invert_over_copy"] = round(res["invert_ms"] / res["copy_ms"], 3)
    res["copy_GBps"] = round(24.0 * nvox * nt / res["copy_ms"] / 1e6, 1)
    del src, dst
    T2s = np.logspace(np.log10(10.0), np.log10(2000.0), 60)
    plan = pkg.Met2Plan(nt, 60, 91)
    try:
        plan.build_dictionary_epg(T2s, 1000.0 * np.ones(60), 10.0, np.linspace(90.0, 180.0, 91), 3000.0)
        plan.set_penalty("L2", T2s)
        fa = torch.full((nvox,), 90.0, dtype=torch.float64, device=dev)                 # 180 degrees: the decays above are pure exponentials
        kw = dict(fa_index=fa, want_status=False)
        res["fit_ms"] = round(timed(lambda: plan.fit("X2", data, **kw), a.fit_steps, 1), 2)
        res["fit_rician3_ms"] = round(timed(lambda: plan.fit_rician("X2", data, n_iter=3, sigma=sigma, **kw), a.fit_steps, 1), 2)
        res["fit_rician3_sigma_estimated_ms"] = round(timed(lambda: plan.fit_rician("X2", data, n_iter=3, **kw), a.fit_steps, 1), 2)
        res["fit_rician3_over_fit"] = round(res["fit_rician3_ms"] / res["fit_ms"], 3)
    finally:
        plan.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
