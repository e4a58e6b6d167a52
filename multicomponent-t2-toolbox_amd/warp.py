"""Non-linear (deformable) registration and resampling through a displacement field (met2_warp, met2_warp_labels, met2_warp_compose,
met2_warp_max_norm2, met2_warp_lncc in include/met2_hip.h, which states the rules; csrc/met2_warp.hip), the inverse of a field and its
Jacobian determinant (met2_warp_invert_step, met2_warp_jacobian).  The stages run on the device; the loops around them are here.

A displacement field `disp` is fp64 [mx, my, mz, 3] on the fixed (destination) grid, in voxels of that grid: with A of resample.voxel_matrix
(fixed voxel -> moving voxel), fixed voxel x samples the moving image at A (x + disp(x)).

  warp, warp_labels, compose, max_norm2, lncc, lncc_sums, lncc_force, work_bytes   the stage wrappers (numpy in, numpy out; tensors in, tensors out)
  register                                                                      greedy registration, coarse to fine
  invert_step, jacobian                                                         one step of the inverse; the determinant and the count of folded voxels
  invert                                                                        the inverse field by fixed-point iteration

register.  Greedy registration with the squared local normalised cross-correlation (the metric of ANTs' CC and of `greedy -m NCC`): per
iteration the moving image is warped (order 1), the metric force is taken (met2_warp_lncc: ANTs' centre-voxel approximation of the gradient,
not the sum over all windows that hold a voxel), smoothed (sigma_fluid, the fluid regularisation), scaled so that its largest vector is
`step` voxels, composed into the field (phi <- phi o (id + w)), and the field is smoothed (sigma_elastic, the elastic regularisation).  The
iteration counts are fixed: with a constant normalised step the metric is not monotone near the end, so the trace is returned for the user
to judge.  Inside a level nothing is copied from the device to the host.

invert.  With T(x) = A (x + u(x)) the inverse is returned in the same form, v on the moving grid with B = A^-1 (moving voxel y samples the
fixed grid at B (y + v(y))), so warp and warp_labels apply it unchanged.  v solves v(y) = -L u(B (y + v(y))), L the 3 x 3 part of A, iterated
from v = 0 (Chen et al., Med. Phys. 35:81-88, 2008).  The iteration converges only where L u B is a contraction (a Lipschitz constant below
1): greedy LNCC registration with a fixed step does not promise that, so the largest change of every step is returned as `residual`, and
jacobian counts the voxels at which the field folds, for the user to judge.  The number of steps is fixed and nothing is copied to the host
inside the loop.  Beyond the rim of the fixed grid u is taken at the nearest voxel (the clamp of compose); `inside` tells where that happened.

Out of scope: symmetric (SyN) updates, mutual-information forces, the exact LNCC gradient, masks or weights, order 3,
convergence-based stopping.  Parity with ANTs, greedy or fnirt is unpinned: none was available."""
import ctypes as C

import numpy as np

from . import register as _reg
from . import resample
from ._lib import _dp, check, lib

MAX_RADIUS = 4                     # MET2_WARP_MAX_RADIUS
EPS = 1e-10                        # the variance floor of register's force: the images are scaled to [0, 1]
IDENTITY = np.ascontiguousarray(np.eye(4)[:3])


# ---------------------------------------------------------------- the checks, before any device work

def _radius(radius):
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError("radius must lie in 1 .. %d" % MAX_RADIUS)
    return int(radius)


def _eps(eps):
    eps = float(eps)
    if not (np.isfinite(eps) and eps >= 0.0):
        raise ValueError("eps must be finite and not negative")
    return eps


def _field_dims(shape, what="disp"):
    shape = tuple(int(n) for n in shape)
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError("%s must be [mx, my, mz, 3]" % what)
    return _grid(shape[:3], what)


def _grid(shape, what):
    """every grid of a warp obeys the source limits of the resampling: the field lives on the destination"""
    return resample._dims(shape, what, True)


def work_bytes(shape):
    """the bytes of the work space of lncc, lncc_sums and lncc_force on a volume of `shape` (met2_warp_work_bytes; no device needed)"""
    b = C.c_int64(-1)
    check(lib().met2_warp_work_bytes(resample._i3(_grid(shape, "volume")), C.byref(b)))
    return b.value


# ---------------------------------------------------------------- the stage wrappers

def _is_tensor(x):
    import torch
    return torch.is_tensor(x)


def _shape(x):
    return tuple(x.shape) if _is_tensor(x) else np.shape(x)


def _work(work, need, dev):
    import torch
    if work is None:
        return torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
    if not (torch.is_tensor(work) and work.is_cuda and work.is_contiguous()):
        raise ValueError("work must be a contiguous device tensor")
    return work


def warp(values, A, disp, order=1, cval=0.0, layout="series", device=0, return_inside=False):
    """`values` on the grid of `disp` [mx, my, mz, 3] through A and the field (met2_warp), order 0 or 1; layouts as resample.resample.
    -> the warped values in the layout they came in; return_inside=True: (values, inside [mx, my, mz] uint8)."""
    import torch
    src_dims, S, has_axis = resample._series_shape(_shape(values), layout)
    src_dims = _grid(src_dims, "source")
    dst_dims = _field_dims(_shape(disp))
    a = resample._matrix(A)
    if isinstance(order, bool) or order not in (0, 1):
        raise ValueError("order must be 0 (nearest) or 1 (trilinear)")
    n_src, n_dst = int(np.prod(src_dims)), int(np.prod(dst_dims))
    svs, sss = resample.check_strides(S, n_src, *resample.layout_strides(layout, S, n_src))
    dvs, dss = resample.check_strides(S, n_dst, *resample.layout_strides(layout, S, n_dst), destination=True)
    t, dev, as_numpy = resample._enter(values, device, torch.float64)
    u = torch.as_tensor(disp, device=dev).to(torch.float64).contiguous()
    out_shape = dst_dims if not has_axis else ((S,) + dst_dims if layout == "series" else dst_dims + (S,))
    out = torch.empty(out_shape, dtype=torch.float64, device=dev)
    inside = torch.empty(dst_dims, dtype=torch.uint8, device=dev) if return_inside else None
    with torch.cuda.device(dev):
        check(lib().met2_warp(dev.index or 0, int(order), resample._i3(src_dims), S, t.data_ptr(), svs, sss, resample._i3(dst_dims), a.ctypes.data_as(_dp),
                              u.data_ptr(), float(cval), out.data_ptr(), dvs, dss, None if inside is None else inside.data_ptr(), resample._stream(dev)))
    return resample._leave((out, inside) if return_inside else out, as_numpy)


def warp_labels(labels, A, disp, fill=0, device=0, return_inside=False):
    """an integer label volume on the grid of `disp` through A and the field, nearest neighbour (met2_warp_labels); `fill` where outside.
    -> int32 [mx, my, mz]; return_inside=True: (labels, inside uint8)."""
    import torch
    kind_ok = (not labels.dtype.is_floating_point and labels.dtype != torch.bool) if torch.is_tensor(labels) else np.asarray(labels).dtype.kind in "iu"
    if not kind_ok:
        raise ValueError("labels must be an integer volume")
    src_dims = _grid(_shape(labels), "source")
    dst_dims = _field_dims(_shape(disp))
    a = resample._matrix(A)
    if not -2 ** 31 <= int(fill) < 2 ** 31:
        raise ValueError("fill must be an int32")
    if not torch.is_tensor(labels):
        lab = np.asarray(labels)
        if lab.size and (int(lab.min()) < -2 ** 31 or int(lab.max()) >= 2 ** 31):
            raise ValueError("labels must fit an int32")
        labels = np.ascontiguousarray(lab).astype(np.int32)
    t, dev, as_numpy = resample._enter(labels, device, torch.int32)
    u = torch.as_tensor(disp, device=dev).to(torch.float64).contiguous()
    out = torch.empty(dst_dims, dtype=torch.int32, device=dev)
    inside = torch.empty(dst_dims, dtype=torch.uint8, device=dev) if return_inside else None
    with torch.cuda.device(dev):
        check(lib().met2_warp_labels(dev.index or 0, resample._i3(src_dims), t.data_ptr(), resample._i3(dst_dims), a.ctypes.data_as(_dp), u.data_ptr(),
                                     int(fill), out.data_ptr(), None if inside is None else inside.data_ptr(), resample._stream(dev)))
    return resample._leave((out, inside) if return_inside else out, as_numpy)


def compose(u_src, shape, A=None, gain=(1.0, 1.0, 1.0), v=None, step=1.0, vmax2=None, device=0):
    """met2_warp_compose: out(x) = w + gain * u_src(clamp(A (x + w))) on the grid `shape`, w = s v(x) with s = step / sqrt(vmax2) (0 where
    vmax2 is 0; `step` where vmax2 is None; w = 0 where v is None).  vmax2: a one-element device tensor (max_norm2 gives it) or a number.
    A=None: the identity.  -> [mx, my, mz, 3]."""
    import torch
    src_dims = _field_dims(_shape(u_src), "u_src")
    dst_dims = _grid(shape, "destination")
    a = resample._matrix(IDENTITY if A is None else A)
    g = np.ascontiguousarray(np.asarray(gain, dtype=np.float64).reshape(-1))
    if g.shape != (3,) or not np.isfinite(g).all() or not np.isfinite(float(step)):
        raise ValueError("gain must hold three finite factors and step must be finite")
    if v is not None and tuple(_shape(v)) != dst_dims + (3,):
        raise ValueError("v must be [mx, my, mz, 3] on the destination grid")
    t, dev, as_numpy = resample._enter(u_src, device, torch.float64)
    vv = None if v is None else torch.as_tensor(v, device=dev).to(torch.float64).contiguous()
    m2 = None if vmax2 is None else (vmax2 if torch.is_tensor(vmax2) else torch.as_tensor(np.asarray(vmax2, dtype=np.float64))).to(dev, torch.float64).reshape(1)
    out = torch.empty(dst_dims + (3,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_warp_compose(dev.index or 0, resample._i3(src_dims), t.data_ptr(), resample._i3(dst_dims), a.ctypes.data_as(_dp), g.ctypes.data_as(_dp),
                                      None if vv is None else vv.data_ptr(), float(step), None if m2 is None else m2.data_ptr(), out.data_ptr(),
                                      resample._stream(dev)))
    return resample._leave(out, as_numpy)


def max_norm2(v, device=0):
    """max over the voxels of |v|^2 (met2_warp_max_norm2) -> a one-element device tensor for a tensor, a float for numpy"""
    import torch
    _field_dims(_shape(v), "v")
    t, dev, as_numpy = resample._enter(v, device, torch.float64)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_warp_max_norm2(dev.index or 0, t.numel() // 3, t.data_ptr(), out.data_ptr(), resample._stream(dev)))
    return float(out.cpu()[0]) if as_numpy else out


def _lncc_in(fixed, warped, inside, device):
    import torch
    dims = _grid(_shape(fixed), "volume")
    if tuple(_shape(warped)) != dims or tuple(_shape(inside)) != dims:
        raise ValueError("fixed, warped and inside must have one shape")
    f, dev, as_numpy = resample._enter(fixed, device, torch.float64)
    w = torch.as_tensor(warped, device=dev).to(torch.float64).contiguous()
    m = (torch.as_tensor(inside, device=dev) != 0).to(torch.uint8).contiguous()
    return dims, f, w, m, dev, as_numpy


def lncc_sums(fixed, warped, inside, radius, device=0, work=None):
    """the six box sums of met2_warp_lncc (met2_warp_lncc_sums) -> [6, nx, ny, nz]: n, sF, sW, sFF, sWW, sFW"""
    import torch
    radius = _radius(radius)
    dims, f, w, m, dev, as_numpy = _lncc_in(fixed, warped, inside, device)
    wk = _work(work, work_bytes(dims), dev)
    sums = torch.empty((6,) + dims, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_warp_lncc_sums(dev.index or 0, resample._i3(dims), f.data_ptr(), w.data_ptr(), m.data_ptr(), radius, sums.data_ptr(), wk.data_ptr(),
                                        wk.numel() * 8, resample._stream(dev)))
    return resample._leave(sums, as_numpy)


def lncc_force(fixed, warped, inside, sums, eps=EPS, device=0, work=None):
    """the force and the metric from given sums (met2_warp_lncc_force) -> (force [nx, ny, nz, 3], metric [2] = (sum of cc, n valid))"""
    import torch
    eps = _eps(eps)
    dims, f, w, m, dev, as_numpy = _lncc_in(fixed, warped, inside, device)
    if tuple(_shape(sums)) != (6,) + dims:
        raise ValueError("sums must be [6, nx, ny, nz]")
    s = torch.as_tensor(sums, device=dev).to(torch.float64).contiguous()
    wk = _work(work, work_bytes(dims), dev)
    force = torch.empty(dims + (3,), dtype=torch.float64, device=dev)
    metric = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_warp_lncc_force(dev.index or 0, resample._i3(dims), f.data_ptr(), w.data_ptr(), m.data_ptr(), s.data_ptr(), eps, force.data_ptr(),
                                         metric.data_ptr(), wk.data_ptr(), wk.numel() * 8, resample._stream(dev)))
    return resample._leave((force, metric), as_numpy)


def lncc(fixed, warped, inside, radius, eps=EPS, device=0, work=None, metric=None):
    """the metric force (met2_warp_lncc) -> (force [nx, ny, nz, 3], metric [2] = (sum of cc over the valid voxels, their number)); `metric`:
    a two-element device tensor to write into (a row of a level's trace)"""
    import torch
    radius, eps = _radius(radius), _eps(eps)
    dims, f, w, m, dev, as_numpy = _lncc_in(fixed, warped, inside, device)
    wk = _work(work, work_bytes(dims), dev)
    force = torch.empty(dims + (3,), dtype=torch.float64, device=dev)
    metric = torch.empty(2, dtype=torch.float64, device=dev) if metric is None else metric
    with torch.cuda.device(dev):
        check(lib().met2_warp_lncc(dev.index or 0, resample._i3(dims), f.data_ptr(), w.data_ptr(), m.data_ptr(), radius, eps, force.data_ptr(),
                                   metric.data_ptr(), wk.data_ptr(), wk.numel() * 8, resample._stream(dev)))
    return resample._leave((force, metric), as_numpy)


# ---------------------------------------------------------------- the inverse of a field and the Jacobian determinant

def _matrix33(N, what="N"):
    n = np.ascontiguousarray(np.asarray(N, dtype=np.float64))
    if n.shape != (3, 3) or not np.isfinite(n).all():
        raise ValueError("%s must be a finite 3 x 3 matrix" % what)
    return n


def _scalar_out(t, what):
    import torch
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.numel() == 1 and t.is_contiguous()):
        raise ValueError("%s must be a one-element float64 device tensor" % what)
    return t


def _step_into(dev, src_dims, u, dst_dims, b, n, v_in, v_out, inside, res2):
    """met2_warp_invert_step on tensors that are already on `dev`, contiguous and of the right type"""
    import torch
    with torch.cuda.device(dev):
        check(lib().met2_warp_invert_step(dev.index or 0, resample._i3(src_dims), u.data_ptr(), resample._i3(dst_dims), b.ctypes.data_as(_dp),
                                          n.ctypes.data_as(_dp), None if v_in is None else v_in.data_ptr(), v_out.data_ptr(),
                                          None if inside is None else inside.data_ptr(), None if res2 is None else res2.data_ptr(), resample._stream(dev)))


def invert_step(u, B, N, shape, v_in=None, return_inside=False, return_res2=False, res2=None, device=0):
    """met2_warp_invert_step: v_out(y) = N u(clamp(B (y + v_in(y)))) on the grid `shape` (v_in None: zeros), `inside` from the coordinates
    before the clamp, res2 = max |v_out - v_in|^2.  u [nx, ny, nz, 3], B [3, 4], N [3, 3]; an inverse step is B = A^-1, N = -A[:, :3].  res2:
    a one-element float64 device tensor to write into (a row of a loop's trace).
    -> v_out [mx, my, mz, 3]; with return_inside and return_res2 a tuple (v_out, inside uint8, res2: a one-element device tensor for tensors,
    a float for numpy)."""
    import torch
    src_dims = _field_dims(_shape(u), "u")
    dst_dims = _grid(shape, "destination")
    b, n = resample._matrix(B), _matrix33(N)
    if v_in is not None and tuple(_shape(v_in)) != dst_dims + (3,):
        raise ValueError("v_in must be [mx, my, mz, 3] on the destination grid")
    if res2 is not None:
        _scalar_out(res2, "res2")
    t, dev, as_numpy = resample._enter(u, device, torch.float64)
    vv = None if v_in is None else torch.as_tensor(v_in, device=dev).to(torch.float64).contiguous()
    out = torch.empty(dst_dims + (3,), dtype=torch.float64, device=dev)
    inside = torch.empty(dst_dims, dtype=torch.uint8, device=dev) if return_inside else None
    r2 = res2 if res2 is not None else (torch.empty(1, dtype=torch.float64, device=dev) if return_res2 else None)
    _step_into(dev, src_dims, t, dst_dims, b, n, vv, out, inside, r2)
    res = (resample._leave(out, as_numpy),)
    if return_inside:
        res += (resample._leave(inside, as_numpy),)
    if return_res2:
        res += (float(r2.cpu()[0]) if as_numpy else r2,)
    return res if len(res) > 1 else res[0]


def jacobian(disp, scale=1.0, device=0):
    """met2_warp_jacobian: det = scale * det(I + grad u) by central differences, one-sided at the rim, and the number of voxels at which it is
    not > 0 (not-a-number included) -> (det [nx, ny, nz], n_nonpositive: an int for numpy, a one-element int64 device tensor for tensors)"""
    import torch
    dims = _field_dims(_shape(disp))
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError("scale must be finite")
    t, dev, as_numpy = resample._enter(disp, device, torch.float64)
    det = torch.empty(dims, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_warp_jacobian(dev.index or 0, resample._i3(dims), t.data_ptr(), scale, det.data_ptr(), count.data_ptr(), resample._stream(dev)))
    return (det.cpu().numpy(), int(count.cpu()[0])) if as_numpy else (det, count)


def invert(disp, A, shape, n_iter=20, device=0, step=None):
    """The inverse of T(x) = A (x + disp(x)) on the grid `shape` of the moving image, by `n_iter` steps of v <- -L disp(B (y + v)) from v = 0
    (see the module's docstring; it converges only where the field is a contraction).  disp [nx, ny, nz, 3] numpy, A [3, 4] of
    resample.voxel_matrix.  The loop ping-pongs between two device tensors, every step writes its res2 into a row of one device tensor, and
    that tensor is read back once after the loop.  step: a numpy callable with invert_step's meaning -- step(u, B, N, shape, v_in=...,
    return_inside=True, return_res2=True) -> (v_out, inside, res2) -- replaces the device stage: the loop then needs no device.
    -> dict(disp [shape + (3,)] on the destination grid in its voxels, B [3, 4] = A^-1, inside [shape] uint8 from the last step (None with
    n_iter = 0), residual [n_iter] in voxels: the largest change of every step)."""
    src_dims = _field_dims(np.shape(disp))
    dst_dims = _grid(shape, "destination")
    a = resample._matrix(A)
    if abs(np.linalg.det(a[:, :3])) == 0.0:
        raise ValueError("A is singular")
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or int(n_iter) < 0:
        raise ValueError("n_iter must be a count >= 0")
    n_iter = int(n_iter)
    B = np.ascontiguousarray(resample.invert(a)[:3])
    N = np.ascontiguousarray(-a[:, :3])
    if not (np.isfinite(B).all()):
        raise ValueError("the inverse of A is not finite")
    u = np.ascontiguousarray(disp, dtype=np.float64)
    if step is not None:
        if not callable(step):
            raise ValueError("step must be a callable with invert_step's meaning")
        v, inside, rows = None, None, []
        for _ in range(n_iter):
            v, inside, r2 = step(u, B, N, dst_dims, v_in=v, return_inside=True, return_res2=True)
            v = np.ascontiguousarray(v, dtype=np.float64)
            rows.append(float(r2))
        v = np.zeros(dst_dims + (3,)) if v is None else v
        return {"disp": v, "B": B, "inside": None if inside is None else np.asarray(inside, dtype=np.uint8), "residual": np.sqrt(np.asarray(rows, dtype=np.float64))}
    import torch
    dev = torch.device("cuda", device)
    ut = torch.as_tensor(u, device=dev)
    bufs = [torch.zeros(dst_dims + (3,), dtype=torch.float64, device=dev), torch.empty(dst_dims + (3,), dtype=torch.float64, device=dev)]
    inside = torch.empty(dst_dims, dtype=torch.uint8, device=dev) if n_iter else None
    trace = torch.zeros(max(n_iter, 1), dtype=torch.float64, device=dev)
    for k in range(n_iter):
        _step_into(dev, src_dims, ut, dst_dims, B, N, None if k == 0 else bufs[k % 2], bufs[(k + 1) % 2], inside if k == n_iter - 1 else None, trace[k:k + 1])
    return {"disp": bufs[n_iter % 2].cpu().numpy(), "B": B, "inside": None if inside is None else inside.cpu().numpy(),
            "residual": np.sqrt(trace[:n_iter].cpu().numpy())}


# ---------------------------------------------------------------- the loop

STAGE_NAMES = ("warp", "lncc", "smooth", "max_norm2", "compose")


class _HostStages:
    """the five stages as numpy callables (the restatement of tests/tools): warp(moving, A, disp) -> (warped, inside); lncc(fixed, warped,
    inside, radius, eps) -> (force, metric [2]); smooth(field, sigma) -> field; max_norm2(v) -> number; compose(u_src, shape, A, gain, v, step,
    vmax2) -> field"""

    def __init__(self, stages):
        missing = [k for k in STAGE_NAMES if not callable(dict(stages).get(k))]
        if missing:
            raise ValueError("stages must map %s to callables; missing: %s" % (", ".join(STAGE_NAMES), ", ".join(missing)))
        for k in STAGE_NAMES:
            setattr(self, k, stages[k])

    def enter(self, x):
        return np.ascontiguousarray(x, dtype=np.float64)

    def zeros(self, shape):
        return np.zeros(tuple(shape) + (3,))

    def begin_level(self, shape, n_iter):
        pass

    def leave(self, x):
        return np.asarray(x, dtype=np.float64)

    def trace(self, rows):
        return np.asarray(rows, dtype=np.float64).reshape(-1, 2)


class _DeviceStages:
    """the five stages on the device, on tensors; one work block and one smoothing buffer per level, no copy to the host before trace()"""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.work = self.tmp = None

    def enter(self, x):
        return self.torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=self.dev)

    def zeros(self, shape):
        return self.torch.zeros(tuple(shape) + (3,), dtype=self.torch.float64, device=self.dev)

    def begin_level(self, shape, n_iter):
        self.work = self.torch.empty((work_bytes(shape) + 7) // 8, dtype=self.torch.float64, device=self.dev)
        self.tmp = self.torch.empty(tuple(shape) + (3,), dtype=self.torch.float64, device=self.dev)

    def leave(self, x):
        return x.cpu().numpy()

    def trace(self, rows):
        return self.torch.stack(rows).cpu().numpy() if rows else np.zeros((0, 2))

    def warp(self, moving, A, disp):
        return warp(moving, A, disp, order=1, cval=0.0, return_inside=True)

    def lncc(self, fixed, warped, inside, radius, eps):
        return lncc(fixed, warped, inside, radius, eps, work=self.work)

    def smooth(self, field, sigma):
        if not sigma > 0.0:
            return field
        from .filters import gaussian_weights
        torch = self.torch
        rad, w = gaussian_weights(sigma)
        out = torch.empty_like(field)
        tmp = self.tmp if self.tmp is not None and self.tmp.shape == field.shape else torch.empty_like(field)
        with torch.cuda.device(self.dev):
            check(lib().met2_smooth_separable(self.dev.index or 0, *field.shape, rad, w.ctypes.data_as(_dp), field.data_ptr(), out.data_ptr(), tmp.data_ptr(),
                                              resample._stream(self.dev)))     # the weights are read during the call
        return out

    def max_norm2(self, v):
        return max_norm2(v)

    def compose(self, u_src, shape, A, gain, v, step, vmax2):
        return compose(u_src, shape, A, gain, v, step, vmax2)


def register(fixed, fixed_affine, moving, moving_affine, world=None, radius=2, step=0.25, sigma_fluid=1.5, sigma_elastic=0.5, iters=(30, 30, 15),
             scales_mm=None, device=0, stages=None, filters=None):
    """Estimate the displacement field that, after `world` (fixed-world mm -> moving-world mm; register.register estimates one; None: the
    identity), brings `moving` onto `fixed`: numpy volumes [nx, ny, nz] with their voxel-to-world affines.
    Levels: scales_mm, coarse to fine (default 4, 2 and 1 times the fixed image's smallest voxel), `iters` iterations on each; both images go
    through register.pyramid and, per level, register.scale_intensity.  A level with an axis shorter than 2 radius + 2 voxels is skipped.
    The field of a level is carried to the next, and at the end to the fixed image's own grid, by met2_warp_compose.
    radius: of the LNCC window, 1 .. 4; step: the largest displacement of an iteration's update in level voxels; sigma_fluid, sigma_elastic:
    in level voxels, the weights of gaussian_smooth (0: no smoothing).
    stages: a dict of the five stages as numpy callables (see _HostStages) replaces the device stages, `filters` = (smooth, resample) the
    device filters of the pyramid: the run then needs no device.
    -> dict(disp [nx, ny, nz, 3] on the fixed grid in its voxels, world [4, 4], levels: per level that ran dict(scale_mm, shape, iters,
    metric: the mean cc over the valid voxels before every iteration's update))."""
    radius = _radius(radius)
    step, sigma_fluid, sigma_elastic = float(step), float(sigma_fluid), float(sigma_elastic)
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError("step must be a positive number of voxels")
    if not (np.isfinite(sigma_fluid) and sigma_fluid >= 0.0 and np.isfinite(sigma_elastic) and sigma_elastic >= 0.0):
        raise ValueError("sigma_fluid and sigma_elastic must be finite and not negative")
    if max(sigma_fluid, sigma_elastic) > 8.0:
        raise ValueError("sigma_fluid and sigma_elastic may be 8 voxels at the most (a kernel radius of 32)")
    fx, mv = np.asarray(fixed, dtype=np.float64), np.asarray(moving, dtype=np.float64)
    _reg._volume_dims(fx.shape, "fixed")
    _reg._volume_dims(mv.shape, "moving")
    fa, ma = resample._affine44(fixed_affine, "fixed_affine"), resample._affine44(moving_affine, "moving_affine")
    w44 = np.eye(4) if world is None else resample._affine44(world, "world")
    if scales_mm is None:
        scales_mm = [m * _reg.voxel_sizes(fa).min() for m in (4.0, 2.0, 1.0)]
    scales_mm = [float(s) for s in scales_mm]
    if not scales_mm:
        raise ValueError("scales_mm must name one level at least")
    its = [iters] * len(scales_mm) if np.ndim(iters) == 0 else list(iters)
    if len(its) != len(scales_mm) or any(isinstance(n, bool) or int(n) != n or int(n) < 0 for n in its):
        raise ValueError("iters must hold one count >= 0 per level (%d levels)" % len(scales_mm))
    its = [int(n) for n in its]
    if stages is not None and filters is None:
        raise ValueError("stages need `filters` too: the pyramid would run on the device otherwise")
    S = _DeviceStages(device) if stages is None else _HostStages(stages)
    filt = filters if filters is not None else _reg._device_filters(device)
    fx = np.where(np.isfinite(fx), fx, 0.0)
    mv = np.where(np.isfinite(mv), mv, 0.0)
    f_levels = _reg.pyramid(fx, fa, scales_mm, filters=filt)
    m_levels = _reg.pyramid(mv, ma, scales_mm, filters=filt)
    disp, prev_aff, levels = None, None, []
    for (fv, faff), (mvol, maff), scale, n_iter in zip(f_levels, m_levels, scales_mm, its):
        shape = tuple(fv.shape)
        if min(shape) < 2 * radius + 2:
            continue
        S.begin_level(shape, n_iter)
        f, m = S.enter(_reg.scale_intensity(fv)), S.enter(_reg.scale_intensity(mvol))
        A = resample.voxel_matrix(faff, maff, w44)
        disp = S.zeros(shape) if disp is None else _carry(S, disp, prev_aff, faff, shape)
        rows = []
        for _ in range(n_iter):
            warped, inside = S.warp(m, A, disp)
            force, metric = S.lncc(f, warped, inside, radius, EPS)
            rows.append(metric)
            v = S.smooth(force, sigma_fluid)
            disp = S.smooth(S.compose(disp, shape, IDENTITY, (1.0, 1.0, 1.0), v, step, S.max_norm2(v)), sigma_elastic)
        tr = S.trace(rows)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_cc = np.where(tr[:, 1] > 0, tr[:, 0] / tr[:, 1], 0.0)
        levels.append({"scale_mm": scale, "shape": shape, "iters": n_iter, "metric": [float(x) for x in mean_cc]})
        prev_aff = faff
    if disp is None:
        out = np.zeros(fx.shape + (3,))
    elif tuple(disp.shape[:3]) == fx.shape and np.array_equal(prev_aff, fa):
        out = S.leave(disp)
    else:
        out = S.leave(_carry(S, disp, prev_aff, fa, fx.shape))
    return {"disp": np.ascontiguousarray(out, dtype=np.float64), "world": w44, "levels": levels}


def _carry(S, disp, from_affine, to_affine, shape):
    """a field on the grid of from_affine -> the grid `shape` of to_affine (the same axes, other voxels): the values at the new voxels'
    places, clamped at the rim, in the new voxels' units"""
    A = (resample.invert(from_affine) @ to_affine)[:3]
    gain = _reg.voxel_sizes(from_affine) / _reg.voxel_sizes(to_affine)
    return S.compose(disp, tuple(shape), np.ascontiguousarray(A), tuple(gain), None, 0.0, None)
