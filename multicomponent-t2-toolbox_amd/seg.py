"""The stages of the tissue segmentation one by one (met2_seg_consts, met2_seg_init, met2_seg_icm, met2_seg_posterior, met2_seg_finish in
include/met2_hip.h), for tests and diagnostics: they launch the kernels of met2_tissue_segment through the host code met2_tissue_segment
itself runs.  Its first step (domain, log, initial classes, plain EM) is bias.bias_domain / bias_init / bias_em.  The filter itself is
motor.tissue_segment_filter.  numpy in -> numpy out, CUDA tensor in -> tensors out; the small records (constants, classes, partial sums)
are always numpy.  Labels are uint8: a class 0..K-1 on the domain, OFF = 255 off it."""
import ctypes as C

import numpy as np
import torch

from ._lib import _dp, check, lib
from .bias import CHUNK, _dev, _f64, _list, _stream, partial_sum  # noqa: F401

OFF = 255                         # the label of a voxel off the domain
TILE = (4, 8, 16)                 # the tile of seg_icm_kernel in voxels (x, y, z); one thread per z-adjacent pair


def _classes(classes):
    cin = np.ascontiguousarray(np.asarray(classes, dtype=np.float64).reshape(-1))
    if cin.size == 0 or cin.size % 3:
        raise ValueError("classes must be [3 K]")
    return cin, cin.size // 3


def _labels(labels, shape, K, dev):
    ll = torch.as_tensor(labels, device=dev).to(torch.uint8).contiguous()
    if tuple(ll.shape) != tuple(shape):
        raise ValueError("labels must have the shape of y")
    if bool(((ll >= K) & (ll != OFF)).any()):
        raise ValueError("a label must be a class 0..K-1 or 255")
    return ll


def _w3(w):
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
    if w.shape != (3,):
        raise ValueError("w must be (w_x, w_y, w_z)")
    return w


def axis_weights(voxel_size):
    """step 4's w_a = d_min / d_a as the filter's host code makes them.  Needs no GPU."""
    vox = np.asarray(voxel_size, dtype=np.float64).reshape(-1)
    if vox.shape != (3,):
        raise ValueError("voxel_size must be (dx, dy, dz)")
    return vox.min() / vox


def chunk_sums(values):
    """the sums of values [..., N] over chunks of 1024 consecutive entries, [..., np], in the order a first-stage kernel adds them
    (include/met2_hip.h, met2_bias_em): thread h of 256 adds entries h, 256 + h, 512 + h, 768 + h, a butterfly adds the 64 lanes of a wave, the
    four waves add as (0 + 1) + (2 + 3).  On the host in fp64: the same bits as the device's partials when the terms are the same bits."""
    values = np.asarray(values, dtype=np.float64)
    lead, m = values.shape[:-1], values.shape[-1]
    npart = -(-max(m, 1) // CHUNK)
    p = np.zeros(lead + (npart * CHUNK,), dtype=np.float64)
    p[..., :m] = values
    p = p.reshape(lead + (npart, 4, 256))
    a = np.zeros(lead + (npart, 256), dtype=np.float64)
    for j in range(4):
        a = a + p[..., j, :]
    a = a.reshape(lead + (npart, 4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ o]
    w = a[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def seg_consts(classes, device=0):
    """step 2 from classes [3 K] = mu, var, pi -> (a [K] = 1 / (2 var), h [K] = log(var) / 2, live [K] bool)"""
    cin, K = _classes(classes)
    a, h = np.full(K, np.nan), np.full(K, np.nan)
    live = np.full(K, -1, dtype=np.int32)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        check(lib().met2_seg_consts(dev.index or 0, K, cin.ctypes.data_as(_dp), a.ctypes.data_as(_dp), h.ctypes.data_as(_dp),
                                    live.ctypes.data_as(C.POINTER(C.c_int32)), _stream(dev)))
    return a, h, live != 0


def seg_init(y, idx, classes, n_domain=None, device=0):
    """step 3: the first labels on the list idx[0..n_domain), 255 elsewhere -> uint8 shaped like y"""
    as_numpy = not torch.is_tensor(y)
    dev = _dev(y, device)
    yt = _f64(y, dev)
    ii, N = _list(idx, n_domain, yt.numel(), dev)
    cin, K = _classes(classes)
    lab = torch.full(tuple(yt.shape), 7, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_seg_init(dev.index or 0, yt.numel(), yt.data_ptr(), ii.data_ptr(), N, K, cin.ctypes.data_as(_dp), lab.data_ptr(),
                                  _stream(dev)))
    return lab.cpu().numpy() if as_numpy else lab


def seg_icm(labels, y, classes, w=(1.0, 1.0, 1.0), beta=0.1, n_sweeps=1, colour=None, device=0):
    """step 5 on labels [nx,ny,nz] with axis weights w: n_sweeps sweeps (colour None), or the pass of colour 0 or 1 of one sweep -> the new
    labels; `labels` itself is not written"""
    as_numpy = not torch.is_tensor(y)
    dev = _dev(y, device)
    yt = _f64(y, dev)
    if yt.dim() != 3:
        raise ValueError("y must be [nx,ny,nz]")
    cin, K = _classes(classes)
    ll = _labels(labels, yt.shape, K, dev).clone()
    ww = _w3(w)
    if colour is not None and int(colour) not in (0, 1):
        raise ValueError("colour must be 0, 1 or None")
    nx, ny, nz = yt.shape
    with torch.cuda.device(dev):
        check(lib().met2_seg_icm(dev.index or 0, nx, ny, nz, ll.data_ptr(), yt.data_ptr(), K, cin.ctypes.data_as(_dp), ww.ctypes.data_as(_dp),
                                 float(beta), int(n_sweeps), -1 if colour is None else int(colour), _stream(dev)))
    return ll.cpu().numpy() if as_numpy else ll


def seg_posterior(labels, y, idx, classes, w=(1.0, 1.0, 1.0), beta=0.1, n_domain=None, device=0):
    """step 6 -> dict(prob [K, nx, ny, nz] in the order of `classes`, 0 off the list; part [3, K, np]: the partial sums per chunk of the list
    of p_k, p_k y, (p_k d) d; sums [3, K]: those added in the M-step's order)"""
    as_numpy = not torch.is_tensor(y)
    dev = _dev(y, device)
    yt = _f64(y, dev)
    if yt.dim() != 3:
        raise ValueError("y must be [nx,ny,nz]")
    cin, K = _classes(classes)
    ll = _labels(labels, yt.shape, K, dev)
    ii, N = _list(idx, n_domain, yt.numel(), dev)
    ww = _w3(w)
    npart = -(-N // CHUNK)
    part = np.full((3, K, max(npart, 1)), np.nan)
    prob = torch.full((K,) + tuple(yt.shape), float("nan"), dtype=torch.float64, device=dev)
    nx, ny, nz = yt.shape
    with torch.cuda.device(dev):
        check(lib().met2_seg_posterior(dev.index or 0, nx, ny, nz, ll.data_ptr(), yt.data_ptr(), ii.data_ptr(), N, K, cin.ctypes.data_as(_dp),
                                       ww.ctypes.data_as(_dp), float(beta), prob.data_ptr(), part.ctypes.data_as(_dp), _stream(dev)))
    return {"prob": prob.cpu().numpy() if as_numpy else prob, "part": part, "sums": partial_sum(part)}


def seg_finish(labels, prob_raw, classes, device=0):
    """the rank by mu and the relabelling -> (seg uint8 shaped like labels: rank + 1 on the domain, 0 off it; prob [K, ...] in rank order, None
    when prob_raw is None; classes [3 K] in rank order)"""
    as_numpy = not torch.is_tensor(labels)
    dev = _dev(labels, device)
    cin, K = _classes(classes)
    ll = _labels(labels, tuple(labels.shape) if torch.is_tensor(labels) else np.shape(labels), K, dev)
    pr = None
    if prob_raw is not None:
        pr = _f64(prob_raw, dev)
        if tuple(pr.shape) != (K,) + tuple(ll.shape):
            raise ValueError("prob_raw must be [K] + the shape of labels")
    seg = torch.full_like(ll, 99)
    prob = None if pr is None else torch.full_like(pr, float("nan"))
    cout = np.full(3 * K, np.nan)
    with torch.cuda.device(dev):
        check(lib().met2_seg_finish(dev.index or 0, ll.numel(), ll.data_ptr(), None if pr is None else pr.data_ptr(), K, cin.ctypes.data_as(_dp),
                                    seg.data_ptr(), None if prob is None else prob.data_ptr(), cout.ctypes.data_as(_dp), _stream(dev)))
    if as_numpy:
        seg, prob = seg.cpu().numpy(), None if prob is None else prob.cpu().numpy()
    return seg, prob, cout
