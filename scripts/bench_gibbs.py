"""Time of the Gibbs-ringing filter (met2_degibbs, motor.gibbs_filter) on a full-size volume: configs[1]'s geometry, 128 x 128 x 64 voxels of
32 echoes, the default parameters (nshifts 20, windows 1..3).  The volume is a two-pool decay with a sharp-edged ellipse in every slice,
truncated in k-space to 3/4 of the matrix so that it rings, plus Gaussian noise.  HIP events around each call (the entry is blocking: it
allocates and frees its work space inside the call, which the time includes), the warm-up calls discarded.  One JSON line: the median and the
best time, voxels/s, the multiply-adds of the contract (41 n^2 per line for the shifted lines, 12 n^3 per slice for the dense 2-D split) and
the rate they correspond to, and what the filter did (the share of samples moved along x, the RMS change).
--mode 3d times the 3-D filter (met2_degibbs3d, gibbs_filter(mode='3d')) on the same geometry: the edge is then an ellipsoid and the k-space
truncation takes in z; the counts are 41 n^2 per line along each of the three axes and 12 nx + 12 ny + 6 nz per sample for the dense 3-D
split (forward real -> complex along z, complex along y and x; two parts back along x and y and complex -> real along z)."""
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


def volume(dims, nt, noise, seed, three_d=False):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    nx, ny, nz = dims
    ax = [torch.linspace(-1.0, 1.0, n, dtype=torch.float64, device=dev) for n in dims]
    gx, gy, gz = torch.meshgrid(*ax, indexing="ij")
    inside = ((gx / 0.7) ** 2 + (gy / 0.55) ** 2 + ((gz / 0.8) ** 2 if three_d else 0.0) <= 1.0).to(torch.float64)[..., None]
    te = 10.0 * torch.arange(1, nt + 1, dtype=torch.float64, device=dev)
    f = (0.15 + 0.05 * gz)[..., None]
    s = 1000.0 * inside * (f * torch.exp(-te / 20.0) + (1.0 - f) * torch.exp(-te / 80.0)) + 50.0
    F = torch.fft.fft2(s, dim=(0, 1))
    kx = torch.fft.fftfreq(nx, 1.0 / nx, device=dev).abs() <= 3 * nx // 8
    ky = torch.fft.fftfreq(ny, 1.0 / ny, device=dev).abs() <= 3 * ny // 8
    F = F * (kx[:, None] & ky[None, :])[..., None, None]
    if three_d:
        kz = torch.fft.fftfreq(nz, 1.0 / nz, device=dev).abs() <= 3 * nz // 8
        F = torch.fft.fft(F, dim=2) * kz[None, None, :, None]
        F = torch.fft.ifft(F, dim=2)
    s = torch.fft.ifft2(F, dim=(0, 1)).real
    return (s + noise * torch.randn(s.shape, dtype=torch.float64, device=dev, generator=g)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=(128, 128, 64))
    ap.add_argument("--nt", type=int, default=32)
    ap.add_argument("--nshifts", type=int, default=20)
    ap.add_argument("--noise", type=float, default=5.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=("2d", "3d"), default="2d")
    args = ap.parse_args()
    motor = importlib.import_module(PKG + ".motor")
    dims = tuple(args.dims)
    three_d = args.mode == "3d"
    mode = {"mode": "3d"} if three_d else {}                          # the 2-D call is the one without the keyword
    d = volume(dims, args.nt, args.noise, 20260114, three_d)
    for _ in range(args.warmup):
        motor.gibbs_filter(d, nshifts=args.nshifts, **mode)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, sx, sy = motor.gibbs_filter(d, nshifts=args.nshifts, return_shifts=True, **mode)[:3]
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    nx, ny, nz = dims
    nvox = nx * ny * nz
    slices = nz * args.nt
    nj = 2 * args.nshifts + 1
    fma_lines = slices * nj * (ny * nx * nx + nx * ny * ny)              # ny lines of nx samples and nx lines of ny samples per slice
    fma_split = slices * (6 * nx * ny * ny + 8 * nx * nx * ny)           # rows real -> complex, columns forward and back, rows complex -> real
    hbm = slices * nx * ny * 150
    if three_d:
        fma_lines = args.nt * nj * nvox * (nx + ny + nz)
        fma_split = args.nt * nvox * (12 * nx + 12 * ny + 6 * nz)
        hbm = args.nt * nvox * 441                                       # gather 16, the forward passes 24 + 32 + 32, the filter 48, the inverse passes 4 x 32 + 24 + 48, the line passes 17 + 25 + 25, scatter 22
    t = float(np.median(ms)) * 1e-3
    print(json.dumps({"kernel": "degibbs3d" if three_d else "degibbs", "ms_all": [round(m, 3) for m in ms], "dims": list(dims), "nt": args.nt, "nshifts": args.nshifts, "noise": args.noise, "steps": args.steps,
                      "warmup": args.warmup, "ms": round(t * 1e3, 3), "ms_best": round(float(np.min(ms)), 3),
                      "voxels_per_s": round(nvox / t, 1), "gfma_lines": round(fma_lines * 1e-9, 2), "gfma_split": round(fma_split * 1e-9, 2),
                      "tflops_fp64": round(2.0 * (fma_lines + fma_split) / t * 1e-12, 3),
                      "hbm_gb": round(hbm * 1e-9, 3),
                      "moved_share_x": round(float((sx != 0).double().mean().item()), 4),
                      "rms_change": round(float(torch.sqrt(torch.mean((out - d) ** 2)).item()), 4)}))


if __name__ == "__main__":
    main()
