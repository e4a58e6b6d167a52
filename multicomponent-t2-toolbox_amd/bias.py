"""The stages of the bias-field correction one by one (met2_bias_weights, met2_bias_domain, met2_bias_init, met2_bias_em, met2_bias_smooth, met2_bias_update,
met2_bias_apply in include/met2_hip.h), for tests and diagnostics: they launch the kernels of met2_bias_field through the host code
met2_bias_field itself runs.  The filter itself is motor.bias_field_filter.  numpy in -> numpy out, CUDA tensor in -> tensors out; the small
records (statistics, histogram, classes, partial sums, the mean of b) are always numpy."""
import ctypes as C

import numpy as np
import torch

from ._lib import _dp, check, lib

CHUNK = 1024                      # list entries per partial sum


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev(x, device):
    return x.device if torch.is_tensor(x) else torch.device("cuda", device)


def _f64(x, dev):
    return torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()


def _list(idx, n_domain, n, dev):
    """idx as int32 on the device, N; the entries trust idx[0..N) to index the volume, so that is checked here"""
    ii = torch.as_tensor(idx, device=dev).to(torch.int32).contiguous().reshape(-1)
    N = ii.numel() if n_domain is None else int(n_domain)
    if N < 0 or N > ii.numel() or N > n:
        raise ValueError("n_domain must lie in 0..len(idx) and 0..n")
    if N and (int(ii[:N].min()) < 0 or int(ii[:N].max()) >= n):
        raise ValueError("idx must hold voxel indices in [0, n)")
    if ii.numel() == 0:
        ii = torch.zeros(1, dtype=torch.int32, device=dev)           # a pointer the entry accepts; nothing reads it at N = 0
    return ii, N


def partial_sum(part):
    """the sum of the partials part[..., np] in the order the second-stage kernels add them (include/met2_hip.h, met2_bias_em), on the host
    in fp64: the same bits as the device's sum"""
    part = np.asarray(part, dtype=np.float64)
    lead, m = part.shape[:-1], part.shape[-1]
    rows = -(-max(m, 1) // 256)
    p = np.zeros(lead + (rows * 256,), dtype=np.float64)
    p[..., :m] = part
    p = p.reshape(lead + (rows, 256))
    a = np.zeros(lead + (256,), dtype=np.float64)
    for r in range(rows):                                            # thread h: partials h, 256 + h, ..
        a = a + p[..., r, :]
    a = a.reshape(lead + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ o]
    w = a[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def bias_weights(voxel_size, fwhm=20.0):
    """step 1 as the filter's host code makes it -> (radii (r_x, r_y, r_z), [w_x, w_y, w_z]).  Needs no GPU."""
    vox = np.ascontiguousarray(np.asarray(voxel_size, dtype=np.float64).reshape(-1))
    if vox.shape != (3,):
        raise ValueError("voxel_size must be (dx, dy, dz)")
    r = np.zeros(3, dtype=np.int32)
    w = np.zeros(3 * 129, dtype=np.float64)
    check(lib().met2_bias_weights(float(fwhm), vox.ctypes.data_as(_dp), r.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(_dp)))
    cuts = np.cumsum([0] + [2 * int(x) + 1 for x in r])
    return tuple(int(x) for x in r), [w[cuts[a]:cuts[a + 1]].copy() for a in range(3)]


def bias_domain(v, mask=None, device=0):
    """-> (y [nx,ny,nz]: log v on the domain and 0 off it, idx [N] int32: the domain's voxel indices in memory order)"""
    as_numpy = not torch.is_tensor(v)
    dev = _dev(v, device)
    dd = _f64(v, dev)
    if dd.dim() != 3 or (mask is not None and tuple(np.shape(mask)) != tuple(dd.shape)):
        raise ValueError("v must be [nx,ny,nz] and mask the same shape")
    mk = None if mask is None else (torch.as_tensor(mask, device=dev) != 0).to(torch.uint8).contiguous()
    y = torch.full_like(dd, float("nan"))
    idx = torch.full((max(dd.numel(), 1),), -1, dtype=torch.int32, device=dev)
    N = C.c_int64(-1)
    nx, ny, nz = dd.shape
    with torch.cuda.device(dev):
        check(lib().met2_bias_domain(dev.index or 0, nx, ny, nz, dd.data_ptr(), None if mk is None else mk.data_ptr(), y.data_ptr(), idx.data_ptr(),
                                     C.byref(N), _stream(dev)))
    if dd.numel() and not bool((idx[N.value:] == -1).all()):
        raise RuntimeError("met2_bias_domain wrote past the domain's size")
    idx = idx[:N.value].clone()
    return (y.cpu().numpy(), idx.cpu().numpy()) if as_numpy else (y, idx)


def bias_init(y, idx, n_class=3, n_domain=None, device=0):
    """the initial classes from y (the volume) over the list idx[0..n_domain) -> dict(lo, hi, mean, degenerate, hist [256], ss_part [np] or None
    when degenerate, classes [3 K])"""
    dev = _dev(y, device)
    yy = _f64(y, dev).reshape(-1)
    ii, N = _list(idx, n_domain, yy.numel(), dev)
    K = int(n_class)
    npart = -(-N // CHUNK)
    stats = np.full(4, np.nan)
    hist = np.zeros(256, dtype=np.uint32)
    part = np.full(max(npart, 1), np.nan)
    classes = np.full(3 * max(K, 0), np.nan)
    with torch.cuda.device(dev):
        check(lib().met2_bias_init(dev.index or 0, yy.numel(), yy.data_ptr(), ii.data_ptr(), N, K, stats.ctypes.data_as(_dp),
                                   hist.ctypes.data_as(C.POINTER(C.c_uint32)), part.ctypes.data_as(_dp), classes.ctypes.data_as(_dp), _stream(dev)))
    deg = bool(stats[3] != 0.0)
    return {"lo": stats[0], "hi": stats[1], "mean": stats[2], "degenerate": deg, "hist": hist, "ss_part": None if deg else part[:npart],
            "classes": classes}


def bias_em(y, b, idx, classes, n_em=1, n_domain=None, want_rw=False, device=0):
    """n_em EM steps from `classes` [3 K] = mu, var, pi with u = y - b over the list, then (want_rw) the final E-step's (R, W)
    -> dict(part [3, K, np]: the last E-step's partial sums per chunk, None at n_em = 0; sums [3, K]: those added in the M-step's order;
    classes [3 K]: after the last M-step; rw: an array shaped like y with a last axis of 2, or None)"""
    as_numpy = not torch.is_tensor(y)
    dev = _dev(y, device)
    yt = _f64(y, dev)
    yy, bb = yt.reshape(-1), _f64(b, dev).reshape(-1)
    if bb.numel() != yy.numel():
        raise ValueError("b must have the shape of y")
    ii, N = _list(idx, n_domain, yy.numel(), dev)
    cin = np.ascontiguousarray(np.asarray(classes, dtype=np.float64).reshape(-1))
    if cin.size == 0 or cin.size % 3:
        raise ValueError("classes must be [3 K]")
    K = cin.size // 3
    npart = -(-N // CHUNK)
    part = np.full((3, K, max(npart, 1)), np.nan)
    cout = np.full(3 * K, np.nan)
    rw = torch.full(tuple(yt.shape) + (2,), float("nan"), dtype=torch.float64, device=dev) if want_rw else None
    with torch.cuda.device(dev):
        check(lib().met2_bias_em(dev.index or 0, yy.numel(), yy.data_ptr(), bb.data_ptr(), ii.data_ptr(), N, K, cin.ctypes.data_as(_dp), int(n_em),
                                 part.ctypes.data_as(_dp), cout.ctypes.data_as(_dp), None if rw is None else rw.data_ptr(), _stream(dev)))
    if int(n_em) < 1:
        part = None
    if rw is not None and as_numpy:
        rw = rw.cpu().numpy()
    return {"part": part, "sums": None if part is None else partial_sum(part), "classes": cout, "rw": rw}


def bias_smooth(a, radii, weights, axis=None, device=0):
    """`a` [nx,ny,nz,2] through the pass of one axis (axis = 0, 1, 2) or all three in turn (None), with radii (r_x, r_y, r_z) and weights, a
    sequence of the three vectors w_a [2 r_a + 1]"""
    as_numpy = not torch.is_tensor(a)
    dev = _dev(a, device)
    aa = _f64(a, dev)
    if aa.dim() != 4 or aa.shape[3] != 2:
        raise ValueError("a must be [nx,ny,nz,2]")
    r = np.ascontiguousarray(np.asarray(radii, dtype=np.int32).reshape(-1))
    if r.shape != (3,) or len(weights) != 3:
        raise ValueError("three radii and three weight vectors")
    ws = [np.asarray(w, dtype=np.float64).reshape(-1) for w in weights]
    if any(w.size != 2 * int(ra) + 1 for w, ra in zip(ws, r)):
        raise ValueError("w_a must hold 2 r_a + 1 weights")
    w = np.ascontiguousarray(np.concatenate(ws))
    if axis is not None and int(axis) not in (0, 1, 2):
        raise ValueError("axis must be 0, 1, 2 or None")
    out = torch.full_like(aa, float("nan"))
    nx, ny, nz = aa.shape[:3]
    with torch.cuda.device(dev):
        check(lib().met2_bias_smooth(dev.index or 0, nx, ny, nz, aa.data_ptr(), r.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(_dp),
                                     -1 if axis is None else int(axis), out.data_ptr(), _stream(dev)))
    return out.cpu().numpy() if as_numpy else out


def bias_update(b, smoothed, idx, n_domain=None, device=0):
    """-> (the new b, shaped like b: b + S_R / S_W where S_W > 0, less its mean over the list there; that mean).  b itself is not written."""
    as_numpy = not torch.is_tensor(b)
    dev = _dev(b, device)
    bb = _f64(b, dev).clone()
    ss = _f64(smoothed, dev)
    if ss.numel() != 2 * bb.numel():
        raise ValueError("smoothed must be b's shape with a last axis of 2")
    ii, N = _list(idx, n_domain, bb.numel(), dev)
    bmean = C.c_double(float("nan"))
    with torch.cuda.device(dev):
        check(lib().met2_bias_update(dev.index or 0, bb.numel(), bb.data_ptr(), ss.data_ptr(), ii.data_ptr(), N, C.byref(bmean), _stream(dev)))
    return (bb.cpu().numpy() if as_numpy else bb), float(bmean.value)


def bias_apply(v, b, device=0):
    """-> (out = v / exp(b) where v is finite, field = exp(b))"""
    as_numpy = not torch.is_tensor(v)
    dev = _dev(v, device)
    vv, bb = _f64(v, dev), _f64(b, dev)
    if vv.shape != bb.shape:
        raise ValueError("b must have the shape of v")
    out, field = torch.full_like(vv, float("nan")), torch.full_like(vv, float("nan"))
    with torch.cuda.device(dev):
        check(lib().met2_bias_apply(dev.index or 0, vv.numel(), vv.data_ptr(), bb.data_ptr(), out.data_ptr(), field.data_ptr(), _stream(dev)))
    return (out.cpu().numpy(), field.cpu().numpy()) if as_numpy else (out, field)
