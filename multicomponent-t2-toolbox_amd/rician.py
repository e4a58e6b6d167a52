"""The kernels of the Rician noise-floor correction one by one (csrc/met2_rician.hip; tests, diagnostics and the driver's rician='direct').
float64 CUDA tensors in, CUDA tensors out; no plan.  With t = A^2 / (2 sigma^2) the mean of a Rician magnitude is
m(A, sigma) = sigma sqrt(pi / 2) [(1 + t) i0e(t / 2) + t i1e(t / 2)]; the bias is b = m - A (include/met2_hip.h has the contract)."""
import ctypes as C

import torch

from ._lib import check, lib
from .plan import _ptr, unflatten, voxel_layout


def _f64(t, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64:
        raise ValueError("%s must be a float64 CUDA tensor (there is no host fallback)" % what)
    return t


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _per_voxel(t, nvox, dtype, what, order, dev):
    if t is None:
        return None
    t = torch.as_tensor(t, device=dev)
    if t.numel() != nvox:
        raise ValueError("%s has %d entries for %d voxels" % (what, t.numel(), nvox))
    if order == "F" and t.dim() > 1:
        t = t.permute(*reversed(range(t.dim())))
    t = t.reshape(-1)
    return (t != 0).to(torch.uint8).contiguous() if dtype == torch.uint8 else t.to(dtype).contiguous()


def bias(A, sigma):
    """b(A, sigma) elementwise (met2_rician_bias): A and sigma of one shape.  A < 0 reads as 0, sigma = 0 gives 0."""
    A, sigma = _f64(A, "A").contiguous(), _f64(sigma, "sigma").contiguous()
    if A.shape != sigma.shape or A.device != sigma.device:
        raise ValueError("A and sigma must have one shape and one device")
    out = torch.empty_like(A)
    with torch.cuda.device(A.device):
        check(lib().met2_rician_bias(A.device.index, A.numel(), _ptr(A), _ptr(sigma), _ptr(out), _stream(A.device)))
    return out


def step(data, model, sigma, mask=None):
    """One correction (met2_rician_step): data [..., n_te] in any layout fit() takes, model [..., n_te] the fit's signal of the same voxels,
    sigma and mask one entry per voxel.  Returns (out, flag): out = data - b(model, sigma_v), shaped like data, and flag (int32 per voxel): 1
    where the corrected voxel would fall out of the fit's gate (first echo <= 0 or echo sum <= 0) and keeps its raw echoes."""
    _f64(data, "data")
    n_te = data.shape[-1]
    data, nvox, vs, es, vol, order = voxel_layout(data, n_te)
    dev = data.device
    model = _f64(model, "model")
    if tuple(model.shape) != tuple(vol) + (n_te,):
        raise ValueError("model must have the shape of data")
    if order == "F" and model.dim() > 2:
        model = model.permute(*(list(reversed(range(model.dim() - 1))) + [model.dim() - 1]))
    model = model.reshape(nvox, n_te).contiguous()
    sigma = _per_voxel(_f64(sigma, "sigma"), nvox, torch.float64, "sigma", order, dev)
    mask = _per_voxel(mask, nvox, torch.uint8, "mask", order, dev)
    out = torch.empty((nvox, n_te), dtype=torch.float64, device=dev)
    flag = torch.empty((nvox,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_rician_step(dev.index, nvox, n_te, _ptr(data), vs, es, _ptr(model), _ptr(sigma), _ptr(mask), _ptr(out), _ptr(flag), _stream(dev)))
    if len(vol) > 1:
        return unflatten(out, vol, order), unflatten(flag, vol, order)
    return out, flag


def invert(data, sigma, mask=None):
    """m^-1(data, sigma_v) per sample (met2_rician_invert): the amplitude whose Rician mean is the sample, 0 for samples at or below the
    floor sigma sqrt(pi / 2); voxels with mask = 0 or sigma = 0 are copied.  data [..., n_te] in any layout fit() takes, sigma and mask one
    entry per voxel; the result is shaped like data.  It treats a sample as the Rician MEAN, which a denoised magnitude only approximates."""
    _f64(data, "data")
    n_te = data.shape[-1]
    data, nvox, vs, es, vol, order = voxel_layout(data, n_te)
    dev = data.device
    sigma = _per_voxel(_f64(sigma, "sigma"), nvox, torch.float64, "sigma", order, dev)
    mask = _per_voxel(mask, nvox, torch.uint8, "mask", order, dev)
    out = torch.empty((nvox, n_te), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_rician_invert(dev.index, nvox, n_te, _ptr(data), vs, es, _ptr(sigma), _ptr(mask), _ptr(out), _stream(dev)))
    return unflatten(out, vol, order) if len(vol) > 1 else out
