"""Drop-ins for flip_angle_algorithms/fa_estimation.py."""
import ctypes as C

import numpy as np
import torch

from ._cache import plan_for
from ._lib import check, lib


def _fa_batch(plan, data, mask):
    fa, km, _ = plan.fa_bruteforce(torch.as_tensor(np.ascontiguousarray(data, dtype=np.float64), device=plan.device),
                                   None if mask is None else torch.as_tensor(np.asarray(mask) > 0, device=plan.device))
    return fa.cpu().numpy(), km.cpu().numpy()


def compute_optimal_FA(M, Dic_3D, alpha_values):
    """fa_estimation.py:74-90 -> (index, alpha, km, SSE, f)"""
    M = np.ascontiguousarray(M, dtype=np.float64)
    if not np.isfinite(M).all():
        raise ValueError("array must not contain infs or NaNs")
    plan = plan_for(Dic_3D)
    idx, km = _fa_batch(plan, M[None, :], None)
    i = int(idx[0])
    # f and SSE at the selected flip angle: one plain NNLS with that kernel
    out = plan.fit("NNLS", torch.as_tensor(M[None, :], device=plan.device), fa_index=torch.tensor([float(i)], device=plan.device),
                   want_maps=False)
    f = out["fsol"][0].cpu().numpy()
    sse = float(np.sum((out["sig"][0].cpu().numpy() - M) ** 2))
    return i, alpha_values[i], float(np.sum(f)), sse, f


def fitting_slice_FA_brute_force(mask_1d, data_1d, nx, Dic_3D, alpha_values):
    """fa_estimation.py:92-111 -> (FA[nx], FA_index[nx], KM[nx], sum of spectra).  (The reference's own
    function raises NameError on Python 3 -- `xrange`, fa_estimation.py:99; this is its intended result.)"""
    plan = plan_for(Dic_3D)
    data = np.ascontiguousarray(data_1d, dtype=np.float64)
    idx, km = _fa_batch(plan, data, mask_1d)
    fitted = (np.asarray(mask_1d) > 0) & (data.sum(axis=1) > 0)
    FA = np.where(fitted, np.asarray(alpha_values)[idx.astype(int)], 0.0)
    out = plan.fit("NNLS", torch.as_tensor(data, device=plan.device), fa_index=torch.as_tensor(idx, device=plan.device),
                   mask=torch.as_tensor(fitted, device=plan.device), want_maps=False)
    # NB the FA step does not normalise and does not require M[0] > 0 (fa_estimation.py:100); voxels with
    # M[0] <= 0 but sum > 0 keep their FA index and contribute no spectrum here.
    fsum = out["fsol"].sum(dim=0).cpu().numpy()
    return FA, np.where(fitted, idx, 0.0), np.where(fitted, km, 0.0), fsum


def fitting_slice_FA_spline_method(Dic_3D_LR, Dic_3D, data_1d, mask_1d, alpha_values_spline, nx, alpha_values):
    """fa_estimation.py:35-70 -> (FA[nx], FA_index[nx], KM[nx], sum of spectra)"""
    plan_lr = plan_for(Dic_3D_LR)
    plan = plan_for(Dic_3D)
    data = np.ascontiguousarray(data_1d, dtype=np.float64)
    dd = torch.as_tensor(data, device=plan.device)
    mk = torch.as_tensor(np.asarray(mask_1d) > 0, device=plan.device)
    fa, km, _ = plan.fa_spline(plan_lr, alpha_values_spline, alpha_values, dd, mk)
    idx = fa.cpu().numpy()
    fitted = (np.asarray(mask_1d) > 0) & (data.sum(axis=1) > 0)
    FA = np.where(fitted, np.asarray(alpha_values)[idx.astype(int)], 0.0)
    out = plan.fit("NNLS", dd, fa_index=fa, mask=torch.as_tensor(fitted, device=plan.device), want_maps=False)
    return FA, np.where(fitted, idx, 0.0), np.where(fitted, km.cpu().numpy(), 0.0), out["fsol"].sum(dim=0).cpu().numpy()


def fa_spline_select(residual, alpha_values_spline, alpha_values, data, mask=None, want_xmin=True):
    """fa_estimation.py:54-59 for GIVEN residual curves (met2_fa_spline_select): per voxel the not-a-knot cubic through
    (alpha_values_spline, residual[v]), its bounded-Brent minimiser on [90, 180] and the index of the nearest entry of alpha_values.
    residual [nvox, n_lr] and data [nvox, n_te] are float64 CUDA tensors (data only gates: a voxel is fitted when its echoes sum to
    more than zero and its mask entry is non-zero; the others get index 0 and xmin 0).  Met2Plan.fa_spline computes the residuals
    itself; this is the selection step alone.  Returns (fa_index, xmin or None), float64 CUDA tensors [nvox]."""
    for t, what in ((residual, "residual"), (data, "data")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2:
            raise ValueError("%s must be a 2-D float64 CUDA tensor" % what)
    if residual.shape[0] != data.shape[0] or data.device != residual.device:
        raise ValueError("residual and data must hold the same voxels on one device")
    al = np.ascontiguousarray(alpha_values_spline, dtype=np.float64)
    ah = np.ascontiguousarray(alpha_values, dtype=np.float64)
    if residual.shape[1] != al.shape[0]:
        raise ValueError("residual must be [nvox, %d]" % al.shape[0])
    dev = data.device
    residual, data = residual.contiguous(), data.contiguous()
    nvox = data.shape[0]
    mk = None if mask is None else (torch.as_tensor(mask, device=dev).reshape(-1) != 0).to(torch.uint8).contiguous()
    if mk is not None and mk.numel() != nvox:
        raise ValueError("mask has %d entries for %d voxels" % (mk.numel(), nvox))
    fa = torch.empty((nvox,), dtype=torch.float64, device=dev)
    xmin = torch.empty((nvox,), dtype=torch.float64, device=dev) if want_xmin else None
    dp = C.POINTER(C.c_double)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    with torch.cuda.device(dev):
        check(lib().met2_fa_spline_select(dev.index or 0, nvox, al.shape[0], al.ctypes.data_as(dp), ptr(residual), ah.shape[0], ah.ctypes.data_as(dp),
                                          data.shape[1], ptr(data), ptr(mk), ptr(fa), ptr(xmin), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.current_stream(dev).synchronize()
    return fa, xmin
