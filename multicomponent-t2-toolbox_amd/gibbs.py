"""The stages of the Gibbs-ringing filter one by one (met2_gibbs_tables, met2_gibbs_split, met2_gibbs_split3d, met2_gibbs_lines in
include/met2_hip.h), for tests and diagnostics: they launch the kernels of met2_degibbs and met2_degibbs3d through the host code those run.  The filter itself is
motor.gibbs_filter.  numpy in -> numpy out, CUDA tensor in -> tensors out."""
import numpy as np
import torch

from ._lib import check, lib


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def gibbs_table_cols(nshifts):
    """the row length of the shift-kernel table: 2 nshifts + 1 rounded up to the unringing kernel's pass width"""
    jp = lib().met2_gibbs_table_cols(int(nshifts))
    if jp < 0:
        check(jp)
    return jp


def gibbs_tables(n, nshifts=20, device=0):
    """-> (W [n, n] complex128, the DFT matrix exp(-2 pi i b q / n); c [n, jp] float64, c[r, j] = c_j[r], zero in the padding columns),
    numpy arrays, as gibbs_tables_kernel writes them for an axis of length n"""
    dev = torch.device("cuda", device)
    jp = gibbs_table_cols(nshifts)
    n = int(n)
    W = torch.full((max(n, 0), max(n, 0), 2), float("nan"), dtype=torch.float64, device=dev)
    c = torch.full((max(n, 0), jp), float("nan"), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_gibbs_tables(dev.index or 0, n, int(nshifts), W.data_ptr(), c.data_ptr(), _stream(dev)))
    W = W.cpu().numpy()
    return W[..., 0] + 1j * W[..., 1], c.cpu().numpy()


def gibbs_split(data, device=0):
    """the 2-D split of every (z, echo) slice of `data` [nx,ny,nz,nt] -> (Ix, Iy), the same shape"""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 4:
        raise ValueError("data must be [nx,ny,nz,nt]")
    ix, iy = torch.empty_like(dd), torch.empty_like(dd)
    nx, ny, nz, nt = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_gibbs_split(dev.index or 0, nx, ny, nz, nt, dd.data_ptr(), ix.data_ptr(), iy.data_ptr(), _stream(dev)))
    return (ix.cpu().numpy(), iy.cpu().numpy()) if as_numpy else (ix, iy)


def gibbs_split3d(data, device=0):
    """the 3-D split of every echo volume of `data` [nx,ny,nz,nt] -> (Ix, Iy, Iz), the same shape; Ix + Iy + Iz = data"""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    dd = torch.as_tensor(data, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 4:
        raise ValueError("data must be [nx,ny,nz,nt]")
    parts = tuple(torch.empty_like(dd) for _ in range(3))
    nx, ny, nz, nt = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_gibbs_split3d(dev.index or 0, nx, ny, nz, nt, dd.data_ptr(), parts[0].data_ptr(), parts[1].data_ptr(),
                                       parts[2].data_ptr(), _stream(dev)))
    return tuple(t.cpu().numpy() for t in parts) if as_numpy else parts


def gibbs_lines(lines, nshifts=20, minW=1, maxW=3, device=0):
    """the 1-D operator U on `lines` [nlines, n] -> (out [nlines, n], shift [nlines, n] int8, best [nlines, n]: the total variation of the
    winning candidate, min(TVL, TVR) at the chosen shift)"""
    as_numpy = not torch.is_tensor(lines)
    dev = torch.device("cuda", device) if as_numpy else lines.device
    dd = torch.as_tensor(lines, dtype=torch.float64, device=dev).contiguous()
    if dd.dim() != 2:
        raise ValueError("lines must be [nlines,n]")
    out = torch.empty_like(dd)
    shift = torch.empty(dd.shape, dtype=torch.int8, device=dev)
    best = torch.empty_like(dd)
    nl, n = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_gibbs_lines(dev.index or 0, n, nl, dd.data_ptr(), int(nshifts), int(minW), int(maxW), out.data_ptr(), shift.data_ptr(),
                                     best.data_ptr(), _stream(dev)))
    return tuple(t.cpu().numpy() for t in (out, shift, best)) if as_numpy else (out, shift, best)
