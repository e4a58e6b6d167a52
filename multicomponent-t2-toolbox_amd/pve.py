"""The stages of the partial-volume maps one by one (met2_pve_moments, met2_pve_consts, met2_pve_energy, met2_pve_icm, met2_pve_finish in
include/met2_hip.h), for tests and diagnostics: they launch the kernels of met2_partial_volume through the host code met2_partial_volume
itself runs.  The filter itself is motor.partial_volume_filter.  numpy in -> numpy out, CUDA tensor in -> tensors out; the small records
(moments, constants, tables, partial sums) are always numpy.  Types are uint8: 0..K-1 pure, K + j the mixture of classes j and j + 1,
OFF = 255 off the domain."""
import ctypes as C

import numpy as np
import torch

from ._lib import _dp, check, lib
from .bias import CHUNK, _dev, _f64, _stream, partial_sum  # noqa: F401
from .seg import OFF, TILE, _classes, _w3, axis_weights, chunk_sums  # noqa: F401

N_NODES = 64                      # midpoint nodes of a mixture
_ip = C.POINTER(C.c_int32)


def n_types(K):
    return 2 * int(K) - 1


def _u8(x, shape, dev, what):
    t = torch.as_tensor(x, device=dev).to(torch.uint8).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have the shape of v" % what)
    return t


def _types(types, shape, K, dev):
    tt = _u8(types, shape, dev, "types")
    if bool(((tt >= n_types(K)) & (tt != OFF)).any()):
        raise ValueError("a type must be 0..2K-2 or 255")
    return tt


def pve_moments(v, seg, prob, device=0):
    """step 1 -> dict(classes [3 K] = mu, var, pi in linear intensity; part [3, K, np]: the partial sums per chunk of the list of p_k, p_k v,
    (p_k d) d; sums [3, K]: those added in the second stage's order; n_domain)"""
    dev = _dev(v, device)
    vt = _f64(v, dev)
    st = _u8(seg, vt.shape, dev, "seg")
    pt = _f64(prob, dev)
    if pt.dim() != vt.dim() + 1 or tuple(pt.shape[1:]) != tuple(vt.shape) or not 1 <= pt.shape[0]:
        raise ValueError("prob must be [K] + the shape of v")
    K, n = int(pt.shape[0]), vt.numel()
    nch = -(-max(n, 1) // CHUNK)
    part = np.full((3, K, nch), np.nan)
    cl = np.full(3 * K, np.nan)
    N = C.c_int64(-1)
    with torch.cuda.device(dev):
        check(lib().met2_pve_moments(dev.index or 0, n, vt.data_ptr(), st.data_ptr(), pt.data_ptr(), K, C.byref(N), part.ctypes.data_as(_dp),
                                     cl.ctypes.data_as(_dp), _stream(dev)))
    npart = -(-N.value // CHUNK)
    if not np.all(np.isnan(part[:, :, npart:])):
        raise RuntimeError("met2_pve_moments wrote past the list's chunks")
    part = np.ascontiguousarray(part[:, :, :max(npart, 1)])
    if npart == 0:
        part[:] = 0.0
    return {"classes": cl, "part": part, "sums": partial_sum(part), "n_domain": int(N.value)}


def pve_consts(classes, device=0):
    """steps 2 and 3 from classes [3 K] = mu, var, pi -> (a [K], h [K], live [2K-1] bool, table [K-1, 64, 3] = (m, a, h) per node)"""
    cin, K = _classes(classes)
    a, h = np.full(K, np.nan), np.full(K, np.nan)
    live = np.full(n_types(K), -1, dtype=np.int32)
    tab = np.full((K - 1, N_NODES, 3), np.nan)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        check(lib().met2_pve_consts(dev.index or 0, K, cin.ctypes.data_as(_dp), a.ctypes.data_as(_dp), h.ctypes.data_as(_dp),
                                    live.ctypes.data_as(_ip), tab.ctypes.data_as(_dp), _stream(dev)))
    return a, h, live != 0, tab


def pve_energy(v, seg, classes, device=0):
    """steps 2 to 5 -> (E [2K-1] + v.shape: 0 off the domain, +inf for a dead type; types uint8 shaped like v: the first types, 255 off the
    domain)"""
    as_numpy = not torch.is_tensor(v)
    dev = _dev(v, device)
    vt = _f64(v, dev)
    st = _u8(seg, vt.shape, dev, "seg")
    cin, K = _classes(classes)
    if bool((st > K).any()):
        raise ValueError("seg must be 0..K")
    E = torch.full((n_types(K),) + tuple(vt.shape), float("nan"), dtype=torch.float64, device=dev)
    typ = torch.full(tuple(vt.shape), 7, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_pve_energy(dev.index or 0, vt.numel(), vt.data_ptr(), st.data_ptr(), K, cin.ctypes.data_as(_dp), E.data_ptr(),
                                    typ.data_ptr(), _stream(dev)))
    return (E.cpu().numpy(), typ.cpu().numpy()) if as_numpy else (E, typ)


def pve_icm(types, E, live, w=(1.0, 1.0, 1.0), beta_pv=0.3, n_sweeps=1, colour=None, device=0):
    """step 6 on types [nx,ny,nz] given E [2K-1,nx,ny,nz] and live [2K-1]: n_sweeps sweeps (colour None), or the pass of colour 0 or 1 of one
    sweep -> the new types; `types` itself is not written"""
    as_numpy = not torch.is_tensor(E)
    dev = _dev(E, device)
    Et = _f64(E, dev)
    if Et.dim() != 4 or Et.shape[0] % 2 != 1:
        raise ValueError("E must be [2K-1,nx,ny,nz]")
    K = (int(Et.shape[0]) + 1) // 2
    tt = _types(types, Et.shape[1:], K, dev).clone()
    lv = np.ascontiguousarray(np.asarray(live).reshape(-1) != 0, dtype=np.int32)
    if lv.shape != (n_types(K),):
        raise ValueError("live must be [2K-1]")
    ww = _w3(w)
    if colour is not None and int(colour) not in (0, 1):
        raise ValueError("colour must be 0, 1 or None")
    _, nx, ny, nz = Et.shape
    with torch.cuda.device(dev):
        check(lib().met2_pve_icm(dev.index or 0, nx, ny, nz, tt.data_ptr(), Et.data_ptr(), K, lv.ctypes.data_as(_ip), ww.ctypes.data_as(_dp),
                                 float(beta_pv), int(n_sweeps), -1 if colour is None else int(colour), _stream(dev)))
    return tt.cpu().numpy() if as_numpy else tt


def pve_finish(v, types, classes, device=0):
    """step 7 -> (pve [K] + v.shape, pveseg uint8, mixeltype uint8)"""
    as_numpy = not torch.is_tensor(v)
    dev = _dev(v, device)
    vt = _f64(v, dev)
    cin, K = _classes(classes)
    tt = _u8(types, vt.shape, dev, "types")
    pve = torch.full((K,) + tuple(vt.shape), float("nan"), dtype=torch.float64, device=dev)
    ps = torch.full_like(tt, 99)
    mx = torch.full_like(tt, 99)
    with torch.cuda.device(dev):
        check(lib().met2_pve_finish(dev.index or 0, vt.numel(), vt.data_ptr(), tt.data_ptr(), K, cin.ctypes.data_as(_dp), pve.data_ptr(),
                                    ps.data_ptr(), mx.data_ptr(), _stream(dev)))
    return tuple(t.cpu().numpy() for t in (pve, ps, mx)) if as_numpy else (pve, ps, mx)
