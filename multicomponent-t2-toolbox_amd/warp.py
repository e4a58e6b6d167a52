"""Non-linear (deformable) registration and resampling through a displacement field (met2_warp, met2_warp_labels, met2_warp_compose,
met2_warp_max_norm2, met2_warp_lncc in include/met2_hip.h, which states the rules; csrc/met2_warp.hip).  The five stages run on the device;
the loop around them is here.

A displacement field `disp` is fp64 [mx, my, mz, 3] on the fixed (destination) grid, in voxels of that grid: with A of resample.voxel_matrix
(fixed voxel -> moving voxel), fixed voxel x samples the moving image at A (x + disp(x)).

  warp, warp_labels, compose, max_norm2, lncc, lncc_sums, lncc_force, work_bytes   the stage wrappers (numpy in, numpy out; tensors in, tensors out)
  register                                                                      greedy registration, coarse to fine

register.  Greedy registration with the squared local normalised cross-correlation (the metric of ANTs' CC and of `greedy -m NCC`): per
iteration the moving image is warped (order 1), the metric force is taken (met2_warp_lncc: ANTs' centre-voxel approximation of the gradient,
not the sum over all windows that hold a voxel), smoothed (sigma_fluid, the fluid regularisation), scaled so that its largest vector is
`step` voxels, composed into the field (phi <- phi o (id + w)), and the field is smoothed (sigma_elastic, the elastic regularisation).  The
iteration counts are fixed: with a constant normalised step the metric is not monotone near the end, so the trace is returned for the user
to judge.  Inside a level nothing is copied from the device to the host.

Out of scope: symmetric (SyN) updates and inverse fields, mutual-information forces, the exact LNCC gradient, masks or weights, order 3,
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
