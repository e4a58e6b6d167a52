"""The MP-PCA denoiser with what each of its steps leaves (met2_mppca_stages in include/met2_hip.h), for tests and diagnostics: the kernel of
met2_mppca instantiated a second time, with the patch list, the Gram matrix, the eigen-solver's result and its sweep count copied out.  The
filter itself is motor.mppca_filter.  numpy in -> numpy out, CUDA tensor in -> tensors out."""
import numpy as np
import torch

from ._lib import check, lib

STAGE_KEYS = ("out", "sigma", "rank", "n_patch", "patch", "gram", "eigval", "eigvec", "sweeps")


def mppca_stages(data, mask, window=5, max_sweeps=30, device=0):
    """`data` [nx,ny,nz,nt], `mask` [nx,ny,nz] -> dict of STAGE_KEYS: out, sigma and rank as motor.mppca_filter(return_maps=True) gives them
    (bit for bit at max_sweeps=30), n_patch [nx,ny,nz] int32, patch [nx,ny,nz,window^3] int32 (flat voxel offsets, the first n_patch of each
    are set), gram [nx,ny,nz,nt,nt], eigval [nx,ny,nz,nt] (unsorted), eigvec [nx,ny,nz,nt,nt] (columns) and sweeps [nx,ny,nz] int32.  What a
    voxel does not write (see the header) is zero.  max_sweeps 1..30 caps the eigen-solver: a voxel it stops gets rank -2."""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 4 or tuple(np.shape(mask)) != tuple(dd.shape[:3]):
        raise ValueError("data must be [nx,ny,nz,nt] and mask [nx,ny,nz]")
    mk = (torch.as_tensor(mask, device=dev) != 0).to(torch.uint8).contiguous()
    nx, ny, nz, nt = dd.shape
    vol = (nx, ny, nz)
    w3 = min(max(int(window), 0), 63) ** 3                     # (a window the library refuses is refused below)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    res = {"out": torch.empty_like(dd), "sigma": torch.empty(vol, **f64), "rank": torch.empty(vol, **i32),
           "n_patch": torch.zeros(vol, **i32), "patch": torch.zeros(vol + (w3,), **i32), "gram": torch.zeros(vol + (nt, nt), **f64),
           "eigval": torch.zeros(vol + (nt,), **f64), "eigvec": torch.zeros(vol + (nt, nt), **f64), "sweeps": torch.zeros(vol, **i32)}
    with torch.cuda.device(dev):
        check(lib().met2_mppca_stages(dev.index or 0, nx, ny, nz, nt, dd.data_ptr(), mk.data_ptr(), int(window), res["out"].data_ptr(),
                                      res["sigma"].data_ptr(), res["rank"].data_ptr(), int(max_sweeps), res["n_patch"].data_ptr(),
                                      res["patch"].data_ptr(), res["gram"].data_ptr(), res["eigval"].data_ptr(), res["eigvec"].data_ptr(),
                                      res["sweeps"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return {k: t.cpu().numpy() for k, t in res.items()} if as_numpy else res
