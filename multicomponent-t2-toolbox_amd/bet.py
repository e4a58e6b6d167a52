"""The stages of the brain extraction one by one (met2_bet_mean, met2_bet_stats, met2_bet_mesh, met2_bet_evolve, met2_bet_fill in
include/met2_hip.h), for tests and diagnostics: they launch the kernels of met2_brain_mask through the host code met2_brain_mask itself
runs.  The filter itself is motor.brain_mask_filter.  numpy in -> numpy out, CUDA tensor in -> tensors out."""
import ctypes as C

import numpy as np
import torch

from ._lib import _dp, check, lib

STAT_KEYS = ("t2", "t", "t98", "tm", "cx", "cy", "cz", "r")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _voxel(voxel_size):
    vox = np.ascontiguousarray(np.asarray(voxel_size, dtype=np.float64).reshape(-1))
    if vox.shape != (3,):
        raise ValueError("voxel_size must be (dx, dy, dz)")
    return vox


def bet_mesh(level):
    """the host mesh builder: the icosahedron subdivided `level` times -> (unit vertices [nv, 3], triangles [nt, 3] int32, ring [nv, 6] int32:
    every vertex' neighbours counter-clockwise seen from outside, -1 beyond its degree, deg [nv] int32).  Needs no GPU."""
    level = int(level)
    n = 4 ** min(max(level, 0), 4)
    unit = np.empty((10 * n + 2, 3), dtype=np.float64)
    tris = np.empty((20 * n, 3), dtype=np.int32)
    ring = np.empty((10 * n + 2, 6), dtype=np.int32)
    deg = np.empty(10 * n + 2, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    check(lib().met2_bet_mesh(level, unit.ctypes.data_as(_dp), tris.ctypes.data_as(ip), ring.ctypes.data_as(ip), deg.ctypes.data_as(ip)))
    return unit, tris, ring, deg


def bet_mean(data, device=0):
    """the echo mean of `data` [..., nt] -> [...]"""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() < 2 or dd.shape[-1] < 1:
        raise ValueError("data must be [..., nt]")
    out = torch.empty(dd.shape[:-1], dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_bet_mean(dev.index or 0, out.numel(), dd.shape[-1], dd.data_ptr(), out.data_ptr(), _stream(dev)))
    return out.cpu().numpy() if as_numpy else out


def bet_stats(v, voxel_size, device=0):
    """the robust statistics of the volume `v` [nx,ny,nz] -> dict of STAT_KEYS and 'count', the number of voxels above t"""
    dev = torch.device("cuda", device) if not torch.is_tensor(v) else v.device
    dd = torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 3:
        raise ValueError("v must be [nx,ny,nz]")
    vox = _voxel(voxel_size)
    st = np.zeros(8, dtype=np.float64)
    count = C.c_int64(0)
    nx, ny, nz = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_bet_stats(dev.index or 0, nx, ny, nz, dd.data_ptr(), vox.ctypes.data_as(_dp), st.ctypes.data_as(_dp), C.byref(count),
                                   _stream(dev)))
    out = {k: float(x) for k, x in zip(STAT_KEYS, st)}
    out["count"] = int(count.value)
    return out


def bet_evolve(v, voxel_size, stats, vertices, level, f=0.4, n_iter=1000, device=0):
    """n_iter steps of the surface from `vertices` [nv, 3] (mm) on the volume `v`, with the statistics `stats` (a dict of STAT_KEYS or the 8
    numbers) -> the vertices after them"""
    as_numpy = not torch.is_tensor(vertices)
    dev = torch.device("cuda", device) if not torch.is_tensor(v) else v.device
    dd = torch.as_tensor(v, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 3:
        raise ValueError("v must be [nx,ny,nz]")
    n = 4 ** min(max(int(level), 0), 4)
    xin = torch.as_tensor(vertices, dtype=torch.float64, device=dev).contiguous()
    if 0 <= int(level) <= 4 and tuple(xin.shape) != (10 * n + 2, 3):
        raise ValueError("vertices must be [%d, 3] at level %d" % (10 * n + 2, level))
    vox = _voxel(voxel_size)
    st = np.ascontiguousarray([stats[k] for k in STAT_KEYS] if isinstance(stats, dict) else stats, dtype=np.float64)
    if st.shape != (8,):
        raise ValueError("stats must hold t2, t, t98, tm, COG and r")
    out = torch.empty_like(xin)
    nx, ny, nz = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_bet_evolve(dev.index or 0, nx, ny, nz, dd.data_ptr(), vox.ctypes.data_as(_dp), st.ctypes.data_as(_dp), float(f), int(level),
                                    int(n_iter), xin.data_ptr(), out.data_ptr(), _stream(dev)))
    return out.cpu().numpy() if as_numpy else out


def bet_fill(vertices, triangles, shape, voxel_size, device=0):
    """the voxels of a volume of `shape` whose centres lie inside the closed surface (vertices [nv, 3] in mm, triangles [nt, 3]) -> uint8"""
    as_numpy = not torch.is_tensor(vertices)
    dev = torch.device("cuda", device) if as_numpy else vertices.device
    X = torch.as_tensor(vertices, dtype=torch.float64, device=dev).contiguous()
    T = torch.as_tensor(triangles, device=dev).to(torch.int32).contiguous()
    if X.dim() != 2 or X.shape[1] != 3 or T.dim() != 2 or T.shape[1] != 3 or len(shape) != 3:
        raise ValueError("vertices must be [nv, 3], triangles [nt, 3] and shape (nx, ny, nz)")
    vox = _voxel(voxel_size)
    nx, ny, nz = (int(n) for n in shape)
    mask = torch.empty((nx, ny, nz), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_bet_fill(dev.index or 0, nx, ny, nz, vox.ctypes.data_as(_dp), X.shape[0], X.data_ptr(), T.shape[0], T.data_ptr(),
                                  mask.data_ptr(), _stream(dev)))
        torch.cuda.current_stream(dev).synchronize()                 # the host's voxel size stays alive until here
    return mask.cpu().numpy() if as_numpy else mask
