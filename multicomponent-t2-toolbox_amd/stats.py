"""Per-label statistics of maps and spectra on the device (met2_label_index, met2_label_moments, met2_label_quantiles, met2_label_stats in
include/met2_hip.h, which states the contract): for every label (tissue class, atlas ROI) and every series (a map, a T2 bin of the spectra)
the sample size, the mean, the standard deviation (ddof 1) and quantiles bit-equal to np.quantile(method='linear') over the label's
voxels that are not NaN.  The filter of the drivers is motor.label_stats_filter (tissue_stats='yes').
`values` is series-major [S, nvox] (layout='series': the maps) or voxel-major [nvox, S] (layout='voxel': fsol_4D), read in place;
`labels` [nvox] integers: 0 .. n_label-1 is a member of that label, anything else is not.  numpy arrays or device tensors in, numpy out."""
import ctypes as C

import numpy as np
import torch

from ._lib import _dp, check, lib

CHUNK = 16384                     # MET2_STATS_CHUNK: members per partial sum of the moments
SMALL_N = 1024                    # MET2_STATS_SMALL_N: labels of at most this many members are sorted in LDS, larger ones radix-selected
MAX_LABEL, MAX_SERIES, MAX_Q = 4096, 32768, 16
DEFAULT_Q = (0.025, 0.25, 0.5, 0.75, 0.975)


def limits():
    """(CHUNK, SMALL_N, MAX_LABEL, MAX_SERIES, MAX_Q) as the library was built with (a test holds them against the constants above)"""
    v = [C.c_int32(-1) for _ in range(5)]
    check(lib().met2_label_stats_limits(*[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev(x, device):
    return x.device if torch.is_tensor(x) and x.is_cuda else torch.device("cuda", device)


def _i32(x, dev):
    t = torch.as_tensor(x, device=dev)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError("labels, offset and order must be integers")
    return t.reshape(-1).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()


def _values(values, layout, dev):
    """-> (tensor, nvox, n_series, voxel_stride, series_stride)"""
    if layout not in ("series", "voxel"):
        raise ValueError("layout must be 'series' or 'voxel'")
    t = torch.as_tensor(values, dtype=torch.float64, device=dev).contiguous()
    if t.dim() < 2:
        raise ValueError("values must be [S, nvox] (layout='series') or [nvox, S] (layout='voxel')")
    if layout == "series":
        S, nvox = int(t.shape[0]), int(t[0].numel())
        return t, nvox, S, 1, max(nvox, 1)
    S = int(t.shape[-1])
    return t, int(t.numel() // max(S, 1)), S, max(S, 1), 1


def _q(q):
    qq = np.ascontiguousarray(np.asarray(q, dtype=np.float64).reshape(-1))
    return qq, (qq.ctypes.data_as(_dp) if qq.size else None)


def _members(offset, order, n_label, nvox, dev):
    of = _i32(offset, dev)
    od = _i32(order, dev)
    if of.numel() != int(n_label) + 1:
        raise ValueError("offset must be [n_label + 1]")
    M = int(of[-1]) if of.numel() else 0
    if M < 0 or M > od.numel() or (M and (int(od[:M].min()) < 0 or int(od[:M].max()) >= nvox)):
        raise ValueError("order must hold offset[n_label] voxel indices below nvox")
    return of, od


def label_index(labels, n_label, device=0):
    """-> (offset [n_label + 1] int32, order [offset[-1]] int32): the members' voxel indices by ascending label, then ascending voxel"""
    dev = _dev(labels, device)
    lab = _i32(labels, dev)
    n = lab.numel()
    offset = torch.full((max(int(n_label), 0) + 1,), -1, dtype=torch.int32, device=dev)
    order = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_label_index(dev.index or 0, n, lab.data_ptr(), int(n_label), offset.data_ptr(), order.data_ptr(), _stream(dev)))
    of = offset.cpu().numpy()
    return of, order[:int(of[-1])].cpu().numpy()


def label_moments(values, offset, order, layout="series", device=0):
    """-> [n_label, S, 3] = n, mean, std of the member list (offset, order) of label_index"""
    dev = _dev(values, device)
    t, nvox, S, vs, ss = _values(values, layout, dev)
    L = int(np.size(offset) if not torch.is_tensor(offset) else offset.numel()) - 1
    of, od = _members(offset, order, L, nvox, dev)
    out = torch.full((max(L, 0), S, 3), float("nan"), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_label_moments(dev.index or 0, L, of.data_ptr(), od.data_ptr(), S, t.data_ptr(), vs, ss, out.data_ptr(), _stream(dev)))
    return out.cpu().numpy()


def label_quantiles(values, offset, order, q=DEFAULT_Q, layout="series", device=0):
    """-> [n_label, S, len(q)]: np.quantile(sample, q, method='linear') to the bit"""
    dev = _dev(values, device)
    t, nvox, S, vs, ss = _values(values, layout, dev)
    L = int(np.size(offset) if not torch.is_tensor(offset) else offset.numel()) - 1
    of, od = _members(offset, order, L, nvox, dev)
    qq, qp = _q(q)
    out = torch.full((max(L, 0), S, qq.size), float("nan"), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_label_quantiles(dev.index or 0, L, of.data_ptr(), od.data_ptr(), S, t.data_ptr(), vs, ss, qq.size, qp, out.data_ptr(),
                                         _stream(dev)))
    return out.cpu().numpy()


def label_stats(values, labels, n_label, q=DEFAULT_Q, layout="series", device=0):
    """the three stages in one call -> [n_label, S, 3 + len(q)] = n, mean, std, quantiles"""
    dev = _dev(values, device)
    t, nvox, S, vs, ss = _values(values, layout, dev)
    lab = _i32(labels, dev)
    if lab.numel() != nvox:
        raise ValueError("labels must have one entry per voxel of values")
    qq, qp = _q(q)
    out = torch.full((max(int(n_label), 0), S, 3 + qq.size), float("nan"), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_label_stats(dev.index or 0, nvox, lab.data_ptr(), int(n_label), S, t.data_ptr(), vs, ss, qq.size, qp, out.data_ptr(),
                                     _stream(dev)))
    return out.cpu().numpy()
