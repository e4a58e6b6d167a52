"""denoise='TV' of the driver (motor/motor_recon_met2_real_data.py:293-304): per echo volume
    sigma_est = mean(estimate_sigma(vol));  vol <- denoise_tv_chambolle(vol, weight = 2 sigma_est, eps = 2e-4, max_num_iter = 200)
on the device through `met2_tv_chambolle` (csrc/met2_tv.hip): every echo volume in the same launches, one fused stencil kernel per
Chambolle iteration, the stopping rule applied on the device.  There is no CPU or torch fallback.

PARITY UNPINNED: both functions live in scikit-image (PyWavelets underneath), neither of which is in this image; the kernels restate the
published algorithms in scikit-image's operation order; tests/test_tv.py checks them against an independent numpy restatement."""
import ctypes as C

import numpy as np
import torch

from ._lib import Met2Error, TvGeometry, check, lib


def _layout(data):
    """-> (tensor as it lies in memory, echo_major flag).  A Fortran-ordered [nx,ny,nz,nt] tensor (the order nibabel's arrays have) is
    read in place as [nt][nz][ny][nx]; anything else is made C-contiguous."""
    if data.dim() != 4:
        raise ValueError("data must be [nx,ny,nz,nt]")
    if not data.is_contiguous() and data.permute(3, 2, 1, 0).is_contiguous():
        return data, 1
    return data.contiguous(), 0


def tv_chambolle(data, weight=None, weight_factor=2.0, eps=2.0e-4, max_num_iter=200, poll_every=4, device=0, return_info=False):
    """Every echo volume of data [nx,ny,nz,nt] through denoise_tv_chambolle; `weight` = one weight per echo (array) or None:
    weight_factor x the echo's estimate_sigma.  numpy in -> numpy out, CUDA tensor in -> tensor out (same memory order).
    return_info: also (sigma [nt], iterations [nt]) as numpy arrays."""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    if dev.type != "cuda":
        raise Met2Error("TV denoising runs on the GPU only; there is no CPU fallback")
    dd, echo_major = _layout(torch.as_tensor(data, dtype=torch.float64, device=dev))
    nx, ny, nz, nt = dd.shape
    out = torch.empty_strided(dd.shape, dd.stride(), dtype=torch.float64, device=dev)
    if dd.numel() == 0:
        return (out.cpu().numpy() if as_numpy else out, np.zeros(nt), np.zeros(nt, dtype=np.int32)) if return_info else (out.cpu().numpy() if as_numpy else out)
    L = lib()
    nbytes = int(L.met2_tv_work_bytes(nx, ny, nz, nt, echo_major))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    sig = torch.empty(nt, dtype=torch.float64, device=dev)
    its = torch.empty(nt, dtype=torch.int32, device=dev)
    wp = None
    if weight is not None:
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(weight, dtype=np.float64), (nt,)))
        wp = w.ctypes.data_as(C.POINTER(C.c_double))
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        check(L.met2_tv_chambolle(dev.index or 0, nx, ny, nz, nt, dd.data_ptr(), echo_major, wp, float(weight_factor), float(eps),
                                  int(max_num_iter), int(poll_every), out.data_ptr(), sig.data_ptr(), its.data_ptr(), work.data_ptr(),
                                  nbytes, stream.cuda_stream))
        stream.synchronize()                                         # `work` and the host weights stay alive until here
    res = out.cpu().numpy() if as_numpy else out
    if return_info:
        return res, sig.cpu().numpy(), its.cpu().numpy()
    return res


def tv_launch_info(nx, ny, nz, nt=1, echo_major=0):
    """How met2_tv_chambolle lays a [nx,ny,nz,nt] volume out (met2_tv_launch_info; host only, no GPU): dict of oy, step1, step2, xlen,
    nt1, nt2, nseg, ntiles, c0, c1, c2, sigma_cap, nc -- include/met2_hip.h explains them."""
    g = TvGeometry()
    check(lib().met2_tv_launch_info(int(nx), int(ny), int(nz), int(nt), int(echo_major), C.byref(g)))
    return {k: int(getattr(g, k)) for k, _ in TvGeometry._fields_}


def tv_detail_coefficients(data, device=0):
    """The 'ddd' db2 coefficients estimate_sigma takes its median of, for every echo volume of data [nx,ny,nz,nt] (met2_tv_detail: the
    gather and tv_detail_kernel as met2_tv_chambolle launches them) -> [(nx+3)//2, (ny+3)//2, (nz+3)//2, nt], numpy for numpy, tensor for
    a CUDA tensor.  A Fortran-ordered input is read in place like tv_chambolle's."""
    as_numpy = not torch.is_tensor(data)
    dev = torch.device("cuda", device) if as_numpy else data.device
    if dev.type != "cuda":
        raise Met2Error("TV denoising runs on the GPU only; there is no CPU fallback")
    dd, echo_major = _layout(torch.as_tensor(data, dtype=torch.float64, device=dev))
    nx, ny, nz, nt = dd.shape
    g = tv_launch_info(nx, ny, nz, nt, echo_major)
    coef = torch.empty((nt, g["c0"], g["c1"], g["c2"]), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_tv_detail(dev.index or 0, nx, ny, nz, nt, dd.data_ptr(), echo_major, coef.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    res = coef.permute(3, 2, 1, 0) if echo_major else coef.permute(1, 2, 3, 0)      # memory axis order -> [x, y, z, echo]
    return res.cpu().numpy() if as_numpy else res


def tv_sigma_from_coefficients(coef, weight=None, weight_factor=2.0, device=0):
    """tv_sigma_kernel on coefficients coef [nt, nc] (or [nc]: one echo) supplied by the caller (met2_tv_sigma) -> numpy (sigma [nt],
    weight [nt], copy [nt] int32): median(|d|) / 0.6744897501960817 over the non-zero d, the weight tv_chambolle would use (`weight` per echo if
    given, else weight_factor x sigma) and whether the echo would be copied through."""
    as_numpy = not torch.is_tensor(coef)
    dev = torch.device("cuda", device) if as_numpy else coef.device
    if dev.type != "cuda":
        raise Met2Error("TV denoising runs on the GPU only; there is no CPU fallback")
    cc = torch.as_tensor(coef, dtype=torch.float64, device=dev)
    if cc.dim() == 1:
        cc = cc[None]
    if cc.dim() != 2 or cc.shape[1] < 1 or cc.shape[0] < 1:
        raise ValueError("coef must be [nt, nc]")
    cc = cc.contiguous()
    nt, nc = cc.shape
    sig = torch.empty(nt, dtype=torch.float64, device=dev)
    wout = torch.empty(nt, dtype=torch.float64, device=dev)
    cp = torch.empty(nt, dtype=torch.int32, device=dev)
    wp = None
    if weight is not None:
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(weight, dtype=np.float64), (nt,)))
        wp = w.ctypes.data_as(C.POINTER(C.c_double))
    with torch.cuda.device(dev):
        check(lib().met2_tv_sigma(dev.index or 0, nt, nc, cc.data_ptr(), wp, float(weight_factor), sig.data_ptr(), wout.data_ptr(), cp.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream))
    return sig.cpu().numpy(), wout.cpu().numpy(), cp.cpu().numpy()


def tv_denoise_volume(data, weight_factor=2.0, eps=2.0e-4, max_num_iter=200, return_info=False):
    """motor:293-304 on data [nx, ny, nz, nt]: estimate_sigma + denoise_tv_chambolle for every echo volume.  A nan or inf in the data
    raises like the reference's finite check."""
    res = tv_chambolle(data, None, weight_factor, eps, max_num_iter, return_info=True)
    if weight_factor != 0 and not np.isfinite(res[1]).all():
        raise ValueError("array must not contain infs or NaNs")
    return res if return_info else res[0]
