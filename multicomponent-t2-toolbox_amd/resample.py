"""Affine resampling of volumes and label images on the device (met2_resample, met2_resample_labels, met2_resample_prefilter and
met2_resample_work_bytes in include/met2_hip.h, which states the contract: scipy.ndimage.affine_transform with mode='constant', restated),
and the transform algebra that goes with it, in numpy.  The filters of the drivers are motor.resample_filter, motor.resample_labels_filter
and motor.atlas_stats_filter.

A transform is `A` [3, 4]: destination voxel (i, j, k) lies at the continuous SOURCE voxel coordinates A[:, :3] @ (i, j, k) + A[:, 3].
voxel_matrix makes it from the two images' voxel-to-world affines (nifti.py reads them) and an optional world-to-world matrix; from_flirt and
to_flirt translate such a world matrix from and to FSL's FLIRT convention.  register.py estimates one.

The stage wrappers take `values` series-major [S, nx, ny, nz] (layout='series': maps) or voxel-major [nx, ny, nz, S] (layout='voxel': echo
data, spectra), read in place, and return the same layout on the destination grid; a 3-D volume is one series.  numpy arrays in, numpy out;
device tensors in, tensors out.  A scalar map that is resampled onto a coarser grid aliases: smooth it first (motor.gaussian_smooth)."""
import ctypes as C

import numpy as np

from ._lib import _dp, check, lib

MAX_AXIS = 512                     # MET2_RESAMPLE_MAX_AXIS
MAX_SERIES = 32768                 # MET2_RESAMPLE_MAX_SERIES
ORDERS = (0, 1, 3)


# ---------------------------------------------------------------- the transform algebra (numpy, no device)

def _affine44(m, name):
    a = np.asarray(m, dtype=np.float64)
    if a.shape == (3, 4):
        a = np.vstack([a, [0.0, 0.0, 0.0, 1.0]])
    if a.shape != (4, 4) or not np.isfinite(a).all():
        raise ValueError("%s must be a finite 4 x 4 (or 3 x 4) matrix" % name)
    if not np.array_equal(a[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("%s must be affine: its last row must be (0, 0, 0, 1)" % name)
    if abs(np.linalg.det(a[:3, :3])) == 0.0:
        raise ValueError("%s is singular" % name)
    return a


def invert(world):
    """the inverse of a 4 x 4 affine, its last row exactly (0, 0, 0, 1)"""
    w = _affine44(world, "world")
    out = np.eye(4)
    out[:3, :3] = np.linalg.inv(w[:3, :3])
    out[:3, 3] = -out[:3, :3] @ w[:3, 3]
    return out


def voxel_matrix(dst_affine, src_affine, world=None):
    """-> A [3, 4] = the first three rows of inv(src_affine) @ world @ dst_affine: destination voxel indices -> continuous source voxel
    coordinates.  The affines map voxel indices to world mm (NIfTI sform / qform); `world` [4, 4] takes destination-world mm to source-world
    mm and defaults to the identity: both images then share scanner space."""
    d = _affine44(dst_affine, "dst_affine")
    s = _affine44(src_affine, "src_affine")
    w = np.eye(4) if world is None else _affine44(world, "world")
    return np.ascontiguousarray((invert(s) @ w @ d)[:3])


def _flirt_scaled(affine, shape, name):
    """voxel indices -> FSL's scaled coordinates: the voxel sizes on the diagonal, and the x index flipped to n_x - 1 - i where the affine's
    determinant is positive (FSL keeps a radiological voxel order)"""
    a = _affine44(affine, name)
    if len(shape) < 3 or any(int(n) < 1 for n in shape[:3]):
        raise ValueError("a shape needs three axes of at least one voxel")
    pix = np.sqrt((a[:3, :3] ** 2).sum(axis=0))
    t = np.diag([pix[0], pix[1], pix[2], 1.0])
    if np.linalg.det(a[:3, :3]) > 0:
        t[0, 0] = -pix[0]
        t[0, 3] = pix[0] * (int(shape[0]) - 1)
    return t, a


def from_flirt(mat, src_affine, src_shape, dst_affine, dst_shape):
    """A FLIRT matrix (flirt -omat; `flirt -in <src> -ref <dst>`) -> the `world` matrix of voxel_matrix (destination-world mm -> source-world mm).
    FSL's rule: the matrix maps the moving image (here the source) to the reference (the destination) in coordinates that are the voxel
    indices times the voxel sizes, the x index counted from the other end (n_x - 1 - i) in an image whose affine has a positive determinant.
    Parity with flirt itself is unpinned: FSL was not available; the rule is FSL's published one, checked by hand on one case (tests)."""
    m = _affine44(mat, "mat")
    ts, a_s = _flirt_scaled(src_affine, src_shape, "src_affine")
    td, a_d = _flirt_scaled(dst_affine, dst_shape, "dst_affine")
    return a_s @ invert(ts) @ invert(m) @ td @ invert(a_d)


def to_flirt(world, src_affine, src_shape, dst_affine, dst_shape):
    """the inverse of from_flirt: `world` -> the FLIRT matrix that `flirt -in <src> -ref <dst> -applyxfm -init` would take"""
    w = _affine44(world, "world")
    ts, a_s = _flirt_scaled(src_affine, src_shape, "src_affine")
    td, a_d = _flirt_scaled(dst_affine, dst_shape, "dst_affine")
    return td @ invert(a_d) @ invert(w) @ a_s @ invert(ts)


# ---------------------------------------------------------------- the checks, before any device work

def _dims(shape, what, source):
    d = tuple(int(n) for n in shape)
    if len(d) != 3 or any(n < 1 for n in d):
        raise ValueError("the %s grid must have three axes of at least one voxel" % what)
    if source and any(n > MAX_AXIS for n in d):
        raise ValueError("a source axis may hold at most %d voxels" % MAX_AXIS)
    if d[0] * d[1] * d[2] > 2 ** 31 - 1:
        raise ValueError("the %s grid may hold at most 2^31 - 1 voxels" % what)
    return d


def _matrix(A):
    a = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
    if a.shape != (3, 4) or not np.isfinite(a).all():
        raise ValueError("A must be a finite 3 x 4 matrix (voxel_matrix makes one)")
    return a


def _order(order):
    if isinstance(order, bool) or order not in ORDERS:
        raise ValueError("order must be 0 (nearest), 1 (trilinear) or 3 (cubic B-spline)")
    return int(order)


def layout_strides(layout, n_series, nvox):
    """(voxel_stride, series_stride) in elements of a contiguous array in `layout`"""
    if layout not in ("series", "voxel"):
        raise ValueError("layout must be 'series' ([S, nx, ny, nz]) or 'voxel' ([nx, ny, nz, S])")
    return (1, max(int(nvox), 1)) if layout == "series" else (max(int(n_series), 1), 1)


def check_strides(n_series, nvox, voxel_stride, series_stride, destination=False):
    """the header's rule: strides >= 1, and on the destination no element shared by two (voxel, series) pairs"""
    vs, ss = int(voxel_stride), int(series_stride)
    if vs < 1 or ss < 1:
        raise ValueError("the strides must be positive")
    if destination and n_series > 1 and nvox > 1 and ss < nvox * vs and vs < n_series * ss:
        raise ValueError("the destination strides make two (voxel, series) pairs share an element")
    return vs, ss


def _series_shape(shape, layout):
    """shape of values -> (source dims, n_series, whether a series axis is there)"""
    shape = tuple(int(n) for n in shape)
    if layout not in ("series", "voxel"):
        raise ValueError("layout must be 'series' ([S, nx, ny, nz]) or 'voxel' ([nx, ny, nz, S])")
    if len(shape) == 3:
        return shape, 1, False
    if len(shape) != 4:
        raise ValueError("values must be [nx, ny, nz], [S, nx, ny, nz] (layout='series') or [nx, ny, nz, S] (layout='voxel')")
    dims, S = (shape[1:], shape[0]) if layout == "series" else (shape[:3], shape[3])
    if S < 1 or S > MAX_SERIES:
        raise ValueError("the number of series must lie in 1 .. %d" % MAX_SERIES)
    return dims, S, True


def _i3(d):
    return (C.c_int32 * 3)(*d)


def work_bytes(order, src_shape, n_series=1):
    """(min_bytes, default_bytes) of the work space of an order-3 call (met2_resample_work_bytes; no device needed): max_work_bytes may lie
    anywhere from min_bytes up; both are 0 for orders 0 and 1."""
    d = _dims(src_shape, "source", True)
    lo, dflt = C.c_int64(-1), C.c_int64(-1)
    check(lib().met2_resample_work_bytes(_order(order), _i3(d), int(n_series), C.byref(lo), C.byref(dflt)))
    return lo.value, dflt.value


# ---------------------------------------------------------------- the stage wrappers

def _enter(x, device, dtype):
    import torch
    as_numpy = not torch.is_tensor(x)
    dev = torch.device("cuda", device) if as_numpy or not x.is_cuda else x.device
    return torch.as_tensor(x, device=dev).to(dtype).contiguous(), dev, as_numpy


def _stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def _leave(out, as_numpy):
    if isinstance(out, tuple):
        return tuple(_leave(t, as_numpy) for t in out)
    return out.cpu().numpy() if as_numpy else out


def resample(values, A, shape, order=1, cval=0.0, layout="series", device=0, return_inside=False, max_work_bytes=0):
    """`values` on the grid `shape` = (mx, my, mz) through A, by interpolation of `order`; voxels whose source coordinates lie outside the
    source grid get `cval`.  -> the resampled values in the layout they came in; return_inside=True: (values, inside [mx, my, mz] uint8).
    Order 3 keeps the spline coefficients of a chunk of series in a work space of at most max_work_bytes (0: the library's default, at most
    1 GiB; work_bytes gives the minimum); the result does not depend on it."""
    import torch
    src_dims, S, has_axis = _series_shape(np.shape(values) if not torch.is_tensor(values) else values.shape, layout)
    src_dims = _dims(src_dims, "source", True)
    dst_dims = _dims(shape, "destination", False)
    a = _matrix(A)
    order = _order(order)
    if int(max_work_bytes) < 0:
        raise ValueError("max_work_bytes must not be negative")
    n_src, n_dst = int(np.prod(src_dims)), int(np.prod(dst_dims))
    svs, sss = check_strides(S, n_src, *layout_strides(layout, S, n_src))
    dvs, dss = check_strides(S, n_dst, *layout_strides(layout, S, n_dst), destination=True)
    t, dev, as_numpy = _enter(values, device, torch.float64)
    out_shape = dst_dims if not has_axis else ((S,) + dst_dims if layout == "series" else dst_dims + (S,))
    out = torch.empty(out_shape, dtype=torch.float64, device=dev)
    inside = torch.empty(dst_dims, dtype=torch.uint8, device=dev) if return_inside else None
    with torch.cuda.device(dev):
        check(lib().met2_resample(dev.index or 0, order, _i3(src_dims), S, t.data_ptr(), svs, sss, _i3(dst_dims), a.ctypes.data_as(_dp), float(cval),
                                  out.data_ptr(), dvs, dss, None if inside is None else inside.data_ptr(), int(max_work_bytes), _stream(dev)))
    return _leave((out, inside) if return_inside else out, as_numpy)


def resample_labels(labels, A, shape, fill=0, device=0, return_inside=False):
    """an integer label volume [nx, ny, nz] on the grid `shape` through A, nearest neighbour (the sample at floor(c + 0.5) per axis); `fill`
    where the source coordinates lie outside.  -> int32 [mx, my, mz]; return_inside=True: (labels, inside uint8)."""
    import torch
    kind_ok = (not labels.dtype.is_floating_point and labels.dtype != torch.bool) if torch.is_tensor(labels) else np.asarray(labels).dtype.kind in "iu"
    if not kind_ok:
        raise ValueError("labels must be an integer volume")
    src_dims = _dims(np.shape(labels) if not torch.is_tensor(labels) else labels.shape, "source", True)
    dst_dims = _dims(shape, "destination", False)
    a = _matrix(A)
    if not -2 ** 31 <= int(fill) < 2 ** 31:
        raise ValueError("fill must be an int32")
    if not torch.is_tensor(labels):
        lab = np.asarray(labels)
        if lab.size and (int(lab.min()) < -2 ** 31 or int(lab.max()) >= 2 ** 31):
            raise ValueError("labels must fit an int32")
        labels = np.ascontiguousarray(lab).astype(np.int32)
    t, dev, as_numpy = _enter(labels, device, torch.int32)
    out = torch.empty(dst_dims, dtype=torch.int32, device=dev)
    inside = torch.empty(dst_dims, dtype=torch.uint8, device=dev) if return_inside else None
    with torch.cuda.device(dev):
        check(lib().met2_resample_labels(dev.index or 0, _i3(src_dims), t.data_ptr(), _i3(dst_dims), a.ctypes.data_as(_dp), int(fill), out.data_ptr(),
                                         None if inside is None else inside.data_ptr(), _stream(dev)))
    return _leave((out, inside) if return_inside else out, as_numpy)


def prefilter(values, layout="series", device=0):
    """the cubic B-spline coefficients of every series (met2_resample_prefilter: the stage order 3 runs first) -> [S, nx, ny, nz], or
    [nx, ny, nz] for a 3-D volume"""
    import torch
    src_dims, S, has_axis = _series_shape(np.shape(values) if not torch.is_tensor(values) else values.shape, layout)
    src_dims = _dims(src_dims, "source", True)
    n_src = int(np.prod(src_dims))
    svs, sss = check_strides(S, n_src, *layout_strides(layout, S, n_src))
    t, dev, as_numpy = _enter(values, device, torch.float64)
    coef = torch.empty(((S,) if has_axis else ()) + src_dims, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_resample_prefilter(dev.index or 0, _i3(src_dims), S, t.data_ptr(), svs, sss, coef.data_ptr(), _stream(dev)))
    return _leave(coef, as_numpy)
