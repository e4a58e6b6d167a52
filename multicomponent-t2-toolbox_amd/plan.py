"""Met2Plan: Python face of the C-ABI plan object.  torch is used only for device memory and
streams; every numeric step runs in libmet2_hip.so."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import Options, check, lib

METHODS = {"NNLS": 0, "T2SPARC": 1, "X2": 2, "L_curve": 3, "GCV": 4, "BayesReg": 5}
PENALTIES = {"I": 0, "L1": 1, "L2": 2, "InvT2": 3}
MAP_NAMES = ("MWF", "IEWF", "FWF", "T2_M", "T2_IE", "TWC")
BOOT_QUANTITIES = MAP_NAMES + ("reg",)              # fit_bootstrap's stats [7][5][...]: the six maps and reg_param
BOOT_QUANTITIES_FA = BOOT_QUANTITIES + ("FA",)        # with fa != "fixed" or want_spectrum: met2_fit_bootstrap_fa's stats [8][5][...]
BOOT_STATS = ("mean", "std", "q025", "q500", "q975")
BOOT_FA_MODES = {"fixed": 0, "brute-force": 1, "spline": 2}

_dp = C.POINTER(C.c_double)


def _h(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def voxel_layout(data, n_te):
    """(tensor, nvox, voxel_stride, echo_stride, vol_shape) for the strided C entries: `data` is [..., n_te] (any number of
    leading voxel axes).  C-contiguous input -> strides (n_te, 1), voxels in C order.  Fortran-contiguous input (what nibabel
    hands the reference's driver, motor:167-173) -> strides (1, nvox), voxels in Fortran order: no copy, outputs come back in
    that voxel order (`unflatten` puts them into the volume's shape).  A 2-D voxel list with any positive strides (a slice of a larger
    list) is read in place as well.  Any other layout is made C-contiguous (one copy)."""
    if data.dim() < 2 or data.shape[-1] != n_te:
        raise ValueError("data must be [..., n_te=%d], got %s" % (n_te, tuple(data.shape)))
    vol = tuple(data.shape[:-1])
    nvox = 1
    for d in vol:
        nvox *= int(d)
    if data.is_contiguous():
        return data, nvox, n_te, 1, vol, "C"
    if data.permute(*reversed(range(data.dim()))).is_contiguous():       # (also an echo-major voxel list: a transposed [n_te, nvox] array)
        return data, nvox, 1, nvox, vol, "F"
    if data.dim() == 2 and data.stride(0) > 0 and data.stride(1) > 0:    # a run of voxels cut out of a larger list (either layout): the C entries take any strides
        return data, nvox, int(data.stride(0)), int(data.stride(1)), vol, "C"
    return data.contiguous(), nvox, n_te, 1, vol, "C"


def unflatten_back(t, order):
    """[vol..., k] output of fit() -> flat [nvox, k] in the data's voxel order (a view for order 'F' volumes too)."""
    if order == "C" or t.dim() <= 2:
        return t.reshape(-1, t.shape[-1])
    nd = t.dim() - 1
    return t.permute(*(list(reversed(range(nd))) + [nd])).reshape(-1, t.shape[-1])


def unflatten(t, vol, order, lead=0):
    """View a per-voxel output ([nvox, ...] or, with lead=1, [k, nvox]) with the voxel axis unfolded to `vol`."""
    if order == "C":
        return t.reshape(t.shape[:lead] + tuple(vol) + t.shape[lead + 1:])
    rv = tuple(reversed(vol))
    u = t.reshape(t.shape[:lead] + rv + t.shape[lead + 1:])
    nd = len(vol)
    perm = list(range(lead)) + [lead + nd - 1 - i for i in range(nd)] + list(range(lead + nd, u.dim()))
    return u.permute(*perm)


class Met2Plan:
    """Shared nTE x nT2 x nFA problem on one GPU: dictionary, Gram matrices, penalty, lambda grid."""

    def __init__(self, n_te, n_t2, n_fa, device=0, x2_factor=1.02, t2sparc_lambda=1.8, myelin_T2=40.0, brent_maxfun=0):
        if not torch.cuda.is_available():
            raise _lib.Met2Error("no GPU visible: the MI355X path has no CPU fallback")
        self.n_te, self.n_t2, self.n_fa = int(n_te), int(n_t2), int(n_fa)
        self.device = torch.device("cuda", int(device))
        opt = Options()
        lib().met2_default_options(C.byref(opt))
        opt.device = int(device)
        opt.x2_factor = x2_factor
        opt.t2sparc_lambda = t2sparc_lambda
        opt.t2_myelin_cut = myelin_T2
        opt.brent_maxfun = brent_maxfun
        self._h = C.c_void_p(0)
        check(lib().met2_plan_create(C.byref(self._h), self.n_te, self.n_t2, self.n_fa, C.byref(opt)))
        # the reference's L-curve grid, bit for bit as numpy builds it (motor:248-251); the C default is the same
        # grid through pow() and can differ in the last bit
        lam = np.zeros(50)
        lam[1:] = np.logspace(np.log10(1e-8), np.log10(10.0), num=49, endpoint=True, base=10.0)
        self._lam_grid = None
        self.alpha_values = None                  # the flip angles in degrees, once build_dictionary_epg has set them
        self.slice_profile = None                 # the slice profile build_dictionary_epg was given, if any
        self.set_lambda_grid(lam)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().met2_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- configuration
    def set_options(self, **kw):
        """x2_factor, t2sparc_lambda, brent_xtol, brent_maxfun, t2_myelin_cut, t2_ie_cut, and the lambda-search intervals x2_lo / x2_hi,
        gcv_lo / gcv_hi, bayes_lo / bayes_hi (scipy's fminbound bounds at algorithms.py:219, :280, bayesian_interpolation.py:101)"""
        opt = Options()
        check(lib().met2_plan_get_options(self._h, C.byref(opt)))
        for k, v in kw.items():
            if not hasattr(opt, k):
                raise AttributeError(k)
            setattr(opt, k, v)
        check(lib().met2_plan_set_options(self._h, C.byref(opt)))
        return self

    def get_options(self, *names):
        opt = Options()
        check(lib().met2_plan_get_options(self._h, C.byref(opt)))
        return {k: getattr(opt, k) for k in (names or ("x2_factor", "t2sparc_lambda", "brent_xtol", "brent_maxfun", "t2_myelin_cut", "t2_ie_cut",
                                                           "x2_lo", "x2_hi", "gcv_lo", "gcv_hi", "bayes_lo", "bayes_hi"))}

    def build_dictionary_epg(self, T2s, T1s, tau, alpha_values, TR, slice_profile=None):
        """slice_profile: None (one flip angle per voxel, the reference's dictionary) or the dict of epg.slice_profile -- the dictionary is
        then the weighted sum of the echo trains over the slice (met2_plan_build_dictionary_epg_profile) and alpha_values are the nominal
        refocusing angles at the slice centre; the plan keeps the profile as plan.slice_profile."""
        (_, p2), (_, p1), (_, pa) = _h(T2s), _h(T1s), _h(alpha_values)
        keep = (_h(T2s), _h(T1s), _h(alpha_values))
        if slice_profile is None:
            check(lib().met2_plan_build_dictionary_epg(self._h, keep[0][1], keep[1][1], float(tau), keep[2][1], float(TR), self._stream()))
        else:
            prof = tuple(_h(np.atleast_1d(np.asarray(slice_profile[k], dtype=np.float64))) for k in ("r_exc", "r_ref", "w"))
            n_z = prof[0][0].shape[0]
            if any(a.ndim != 1 or a.shape[0] != n_z for a, _ in prof):
                raise ValueError("slice_profile: r_exc, r_ref and w must be 1-D arrays of one length")
            check(lib().met2_plan_build_dictionary_epg_profile(self._h, keep[0][1], keep[1][1], float(tau), keep[2][1], float(TR), n_z,
                                                               prof[0][1], prof[1][1], prof[2][1], self._stream()))
            slice_profile = {k: a.copy() for k, (a, _) in zip(("r_exc", "r_ref", "w"), prof)}
        self.slice_profile = slice_profile
        self.alpha_values = keep[2][0].copy()
        return self

    def set_dictionary(self, Dic_3D):
        a, p = _h(Dic_3D)
        if a.shape != (self.n_te, self.n_t2, self.n_fa):
            raise ValueError("Dic_3D must be [n_te, n_t2, n_fa] = %s, got %s" % ((self.n_te, self.n_t2, self.n_fa), a.shape))
        check(lib().met2_plan_set_dictionary(self._h, p))
        self.alpha_values = None
        self.slice_profile = None
        return self

    def get_dictionary(self):
        out = np.zeros((self.n_te, self.n_t2, self.n_fa))
        check(lib().met2_plan_get_dictionary(self._h, out.ctypes.data_as(_dp)))
        return out

    def set_penalty(self, penalty, T2s=None):
        if isinstance(penalty, str):
            a, p = _h(T2s if T2s is not None else np.zeros(self.n_t2))
            check(lib().met2_plan_set_penalty(self._h, PENALTIES[penalty], p))
        else:
            a, p = _h(penalty)
            if a.shape != (self.n_t2, self.n_t2):
                raise ValueError("penalty matrix must be [n_t2, n_t2] = %s, got %s" % ((self.n_t2, self.n_t2), a.shape))
            check(lib().met2_plan_set_penalty_dense(self._h, p))
        return self

    def get_penalty(self):
        out = np.zeros((self.n_t2, self.n_t2))
        check(lib().met2_plan_get_penalty(self._h, out.ctypes.data_as(_dp)))
        return out

    def set_lambda_grid(self, lambda_reg):
        a, p = _h(lambda_reg)
        check(lib().met2_plan_set_lambda_grid(self._h, p, a.shape[0]))
        self._lam_grid = a.copy()
        return self

    def set_t2_grid(self, T2s):
        a, p = _h(T2s)
        check(lib().met2_plan_set_t2_grid(self._h, p))
        return self

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- hot path (device tensors in, device tensors out)
    def _check_data(self, data, what="data"):
        if not torch.is_tensor(data) or not data.is_cuda:
            raise ValueError("%s must be a CUDA tensor (the hot path has no host fallback)" % what)
        if data.device != self.device:
            raise ValueError("%s lives on %s but the plan on %s" % (what, data.device, self.device))
        if data.dtype != torch.float64:
            raise ValueError("%s must be float64, got %s" % (what, data.dtype))

    def _per_voxel(self, t, nvox, dtype, what, order="C", vol=None):
        """fa_index / mask arguments -> flat [nvox] tensor in the voxel order of the data layout."""
        if t is None:
            return None
        t = torch.as_tensor(t, device=self.device)
        if t.numel() != nvox:
            raise ValueError("%s has %d entries for %d voxels" % (what, t.numel(), nvox))
        if order == "F" and t.dim() > 1:
            t = t.permute(*reversed(range(t.dim())))
        t = t.reshape(-1)
        return (t != 0).to(torch.uint8).contiguous() if dtype == torch.uint8 else t.to(dtype).contiguous()

    def fit(self, method, data, fa_index=None, mask=None, want_sig=True, want_maps=True, want_status=True, want_lambda=False,
            out=None, sync=True):
        """data [..., n_te] float64 cuda tensor: a voxel list [nvox, n_te] or a volume [nx, ny, nz, n_te], C- or
        Fortran-contiguous (see voxel_layout; neither is copied).  fa_index / mask: one entry per voxel, flat in the data's
        voxel order or shaped like the volume.  Returns a dict of cuda tensors with the voxel axes of `data`.
        sync=False only enqueues the launches on the current stream (met2_fit_enqueue_strided): call finish() before the
        outputs are read on the host; an FA index outside the dictionary is then reported by finish()."""
        if method not in METHODS:
            raise ValueError("unknown reg_method %r" % (method,))
        self._check_data(data)
        data, nvox, vs, es, vol, order = voxel_layout(data, self.n_te)
        dev = self.device
        fa_index = self._per_voxel(fa_index, nvox, torch.float64, "fa_index", order)
        mask = self._per_voxel(mask, nvox, torch.uint8, "mask", order)
        o = out or {}

        def buf(name, shape, dtype=torch.float64):
            t = o.get(name)
            if t is None:
                return torch.empty(shape, dtype=dtype, device=dev)
            if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError("out[%r] must be a contiguous %s tensor of shape %s on %s" % (name, dtype, tuple(shape), dev))
            return t

        fsol = buf("fsol", (nvox, self.n_t2))
        sig = buf("sig", (nvox, self.n_te)) if want_sig else None
        reg = buf("reg", (nvox,))
        lam = buf("lam", (nvox,)) if want_lambda else None
        maps = buf("maps", (6, nvox)) if want_maps else None
        status = buf("status", (nvox,), torch.int32) if want_status else None
        entry = lib().met2_fit_strided if sync else lib().met2_fit_enqueue_strided
        with torch.cuda.device(dev):
            check(entry(self._h, METHODS[method], nvox, _ptr(data), vs, es, _ptr(fa_index), _ptr(mask), _ptr(fsol),
                        _ptr(sig), _ptr(reg), _ptr(lam), _ptr(maps), _ptr(status), self._stream()))
        res = {"fsol": fsol, "sig": sig, "reg": reg, "lam": lam, "maps": maps, "status": status}
        if len(vol) > 1:
            res = {k: (None if t is None else unflatten(t, vol, order, lead=1 if k == "maps" else 0)) for k, t in res.items()}
        return res

    def attach_fa_spline(self, plan_lr, alpha_lr, alpha_hr=None):
        """met2_plan_attach_fa_spline: `plan_lr` holds the coarse-grid dictionary of the spline FA method (motor:237-238) on this plan's
        device, alpha_lr its angles in degrees, alpha_hr this plan's (default: those build_dictionary_epg was given).  plan_lr=None
        detaches.  Needed by fit_bootstrap(fa="spline"); the coarse plan must outlive the attachment."""
        if plan_lr is None:
            check(lib().met2_plan_attach_fa_spline(self._h, None, 0, None, 0, None))
            return self
        if alpha_hr is None:
            alpha_hr = self.alpha_values
        if alpha_hr is None:
            raise ValueError("alpha_hr is needed: the plan's dictionary was not built by build_dictionary_epg")
        (al, pal), (ah, pah) = _h(alpha_lr), _h(alpha_hr)
        check(lib().met2_plan_attach_fa_spline(self._h, plan_lr._h, al.shape[0], pal, ah.shape[0], pah))
        return self

    def fa_stats_degrees(self, fa_stats):
        """fit_bootstrap's fa_stats [5, ...] (index units) -> degrees on the plan's flip-angle grid: mean and quantiles by linear interpolation
        in the index; std times the grid step if the grid is uniform, else nan (a std has no image under a non-linear map).  None when the
        plan does not know its angles."""
        a = self.alpha_values
        if a is None:
            return None
        x = fa_stats.detach().cpu().numpy() if torch.is_tensor(fa_stats) else np.asarray(fa_stats, dtype=np.float64)
        out = np.interp(x, np.arange(a.shape[0], dtype=np.float64), a)
        d = np.diff(a)
        uniform = d.size > 0 and np.allclose(d, d[0], rtol=1e-9, atol=0.0)
        out[1] = x[1] * abs(d[0]) if uniform else np.nan
        return out

    def fit_bootstrap(self, method, data, n_rep=100, seed=0, fa_index=None, mask=None, sigma=None, voxel_id=None, want_sig=True,
                      want_status=True, want_lambda=False, fa="fixed", want_spectrum=False):
        """Per-voxel bootstrap uncertainty (met2_fit_bootstrap; an extension with no counterpart in the reference).  The point fit is
        fit()'s, bit for bit; then every fitted voxel is refitted on n_rep Rician replicates of its fitted signal at its noise level
        (`sigma`, one entry per voxel, or the plain-NNLS estimate of bayesian_interpolation.py:88-93) and the statistics of the metrics
        are returned.  data, fa_index, mask as for fit(); voxel_id: int64 per voxel (default: the voxel's flat index in the data's
        voxel order) -- a voxel's replicates depend on (seed, voxel_id, replicate, echo) alone.  Returns fit()'s dict plus
        stats [7, 5, vol...] (BOOT_QUANTITIES x BOOT_STATS), sigma [vol...] and rep_status [vol...] (OR of the replicates' status bits).
        fa: "fixed" (the default) refits every replicate at the voxel's fa_index, so the spread holds the noise that reaches the spectrum at a
        fixed dictionary slice; "brute-force" / "spline" re-estimate the flip angle on every replicate row (fa_bruteforce; the spline method
        on the coarse plan of attach_fa_spline) and fit it at that index, so the spread also holds the FA step's error -- use it when the
        pipeline estimates the FA per voxel on the unsmoothed data (fa_index still gives the point fit's FA).  want_spectrum: statistics of the
        replicates' spectra per T2 bin.  With fa != "fixed" or want_spectrum the call goes to met2_fit_bootstrap_fa and the result also has
        fa_stats [5, vol...] (the FA index the replicates were fitted with; BOOT_STATS), fa_stats_deg (numpy, degrees; only when the plan
        knows its angles, see fa_stats_degrees) and, with want_spectrum, spec_stats [5, vol..., n_t2]; stats stays [7, 5, vol...]."""
        if method not in METHODS:
            raise ValueError("unknown reg_method %r" % (method,))
        if fa not in BOOT_FA_MODES:
            raise ValueError("fa must be 'fixed', 'brute-force' or 'spline', got %r" % (fa,))
        extended = fa != "fixed" or bool(want_spectrum)
        if not torch.is_tensor(data):
            raise ValueError("data must be a CUDA tensor (the hot path has no host fallback)")
        if data.dtype != torch.float64:
            raise ValueError("data must be float64, got %s" % (data.dtype,))
        if data.dim() < 2 or data.shape[-1] != self.n_te:
            raise ValueError("data must be [..., n_te=%d], got %s" % (self.n_te, tuple(data.shape)))
        n_rep = int(n_rep)
        if not 2 <= n_rep <= 1024:
            raise ValueError("n_rep must lie in [2, 1024], got %d" % n_rep)
        seed = int(seed)
        if not -2 ** 63 <= seed < 2 ** 64:
            raise ValueError("seed must fit in 64 bits")
        if seed >= 2 ** 63:
            seed -= 2 ** 64                                  # the C entry takes the bits as int64_t
        nvox = 1
        for d in data.shape[:-1]:
            nvox *= int(d)
        if sigma is not None:
            sg = sigma if torch.is_tensor(sigma) else torch.as_tensor(np.asarray(sigma, dtype=np.float64))
            if sg.numel() != nvox:
                raise ValueError("sigma has %d entries for %d voxels" % (sg.numel(), nvox))
            if bool((sg < 0).any()) or bool(torch.isnan(sg).any()):
                raise ValueError("sigma must be >= 0")
        if voxel_id is not None:
            vid_n = voxel_id.numel() if torch.is_tensor(voxel_id) else np.asarray(voxel_id).size
            if vid_n != nvox:
                raise ValueError("voxel_id has %d entries for %d voxels" % (vid_n, nvox))
        self._check_data(data)
        data, nvox, vs, es, vol, order = voxel_layout(data, self.n_te)
        dev = self.device
        fa_index = self._per_voxel(fa_index, nvox, torch.float64, "fa_index", order)
        mask = self._per_voxel(mask, nvox, torch.uint8, "mask", order)
        sigma = self._per_voxel(sigma, nvox, torch.float64, "sigma", order)
        vid = self._per_voxel(voxel_id, nvox, torch.int64, "voxel_id", order)
        e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
        fsol, reg, maps = e((nvox, self.n_t2)), e((nvox,)), e((6, nvox))
        sig = e((nvox, self.n_te)) if want_sig else None
        lam = e((nvox,)) if want_lambda else None
        status = e((nvox,), torch.int32) if want_status else None
        sigma_out, stats, rep_status = e((nvox,)), e((8 if extended else 7, 5, nvox)), e((nvox,), torch.int32)
        spec = e((5, nvox, self.n_t2)) if want_spectrum else None
        with torch.cuda.device(dev):
            if extended:
                check(lib().met2_fit_bootstrap_fa(self._h, METHODS[method], BOOT_FA_MODES[fa], nvox, _ptr(data), vs, es, _ptr(fa_index), _ptr(mask),
                                                  _ptr(vid), _ptr(sigma), n_rep, seed, _ptr(fsol), _ptr(sig), _ptr(reg), _ptr(lam), _ptr(maps),
                                                  _ptr(status), _ptr(sigma_out), _ptr(stats), _ptr(spec), _ptr(rep_status), self._stream()))
            else:
                check(lib().met2_fit_bootstrap(self._h, METHODS[method], nvox, _ptr(data), vs, es, _ptr(fa_index), _ptr(mask), _ptr(vid), _ptr(sigma),
                                               n_rep, seed, _ptr(fsol), _ptr(sig), _ptr(reg), _ptr(lam), _ptr(maps), _ptr(status), _ptr(sigma_out),
                                               _ptr(stats), _ptr(rep_status), self._stream()))
        res = {"fsol": fsol, "sig": sig, "reg": reg, "lam": lam, "maps": maps, "status": status, "sigma": sigma_out,
               "stats": stats[:7] if extended else stats,
               "rep_status": rep_status}
        if extended:
            res["fa_stats"] = stats[7]
            if want_spectrum:
                res["spec_stats"] = spec
        if len(vol) > 1:
            lead = {"maps": 1, "stats": 2, "fa_stats": 1, "spec_stats": 1}
            res = {k: (None if t is None else unflatten(t, vol, order, lead=lead.get(k, 0))) for k, t in res.items()}
        if extended and self.alpha_values is not None:
            res["fa_stats_deg"] = self.fa_stats_degrees(res["fa_stats"])
        return res

    def _sigma_arg(self, sigma, nvox, order):
        """sigma of fit_rician: None, one number for every voxel, or one entry per voxel (flat in the data's voxel order or shaped like the volume)"""
        if sigma is None:
            return None
        if not torch.is_tensor(sigma) and np.ndim(sigma) == 0:
            sigma = torch.full((nvox,), float(sigma), dtype=torch.float64, device=self.device)
        sg = sigma if torch.is_tensor(sigma) else torch.as_tensor(np.asarray(sigma, dtype=np.float64))
        if sg.numel() != nvox:
            raise ValueError("sigma has %d entries for %d voxels" % (sg.numel(), nvox))
        if bool((sg < 0).any()) or bool(torch.isnan(sg).any()):
            raise ValueError("sigma must be >= 0")
        return self._per_voxel(sg, nvox, torch.float64, "sigma", order)

    def noise_sigma(self, data, fa_index=None, mask=None, want_sig0=False):
        """The per-voxel noise estimate fit_bootstrap and fit_rician make when no sigma is given (met2_noise_sigma; bayesian_interpolation.py:88-93):
        a plain-NNLS pass at the voxel's flip angle, then sqrt(sum of squared residuals / max(n_te - #{x > 0}, 1)).  data, fa_index, mask as for
        fit().  Returns sigma [vol...], or (sigma, sig0 [vol..., n_te]) with want_sig0 (that pass's model signal)."""
        self._check_data(data)
        data, nvox, vs, es, vol, order = voxel_layout(data, self.n_te)
        fa_index = self._per_voxel(fa_index, nvox, torch.float64, "fa_index", order)
        mask = self._per_voxel(mask, nvox, torch.uint8, "mask", order)
        sigma = torch.empty((nvox,), dtype=torch.float64, device=self.device)
        sig0 = torch.empty((nvox, self.n_te), dtype=torch.float64, device=self.device) if want_sig0 else None
        with torch.cuda.device(self.device):
            check(lib().met2_noise_sigma(self._h, nvox, _ptr(data), vs, es, _ptr(fa_index), _ptr(mask), _ptr(sigma), _ptr(sig0), self._stream()))
        if len(vol) > 1:
            sigma = unflatten(sigma, vol, order)
            sig0 = None if sig0 is None else unflatten(sig0, vol, order)
        return (sigma, sig0) if want_sig0 else sigma

    def fit_rician(self, method, data, n_iter=3, sigma=None, fa_index=None, mask=None, want_sig=True, want_maps=True, want_status=True,
                   want_lambda=False):
        """fit() with the Rician noise floor of the echo magnitudes taken out (met2_fit_rician; an extension with no counterpart in the
        reference): the raw echoes minus the Rician bias b(s_hat, sigma) at the previous fit's model signal s_hat are refitted, n_iter times
        over (0 <= n_iter <= 16; 0 is fit() bit for bit).  sigma: one number, one entry per voxel, or None = noise_sigma() on the raw data; it
        is not re-estimated between the passes.  data, fa_index, mask as for fit().  Returns fit()'s dict -- of the last pass: sig is the
        noise-free signal estimate -- plus sigma [vol...] and rician_flag [vol...] (int32: 1 where the last correction would have pushed the
        voxel out of the fit's gate and it was fitted on its raw echoes).  This is a bias correction around a least-squares fit, not a
        maximum-likelihood Rician fit."""
        if method not in METHODS:
            raise ValueError("unknown reg_method %r" % (method,))
        n_iter = int(n_iter)
        if not 0 <= n_iter <= 16:
            raise ValueError("n_iter must lie in [0, 16], got %d" % n_iter)
        self._check_data(data)
        data, nvox, vs, es, vol, order = voxel_layout(data, self.n_te)
        dev = self.device
        sigma = self._sigma_arg(sigma, nvox, order)
        fa_index = self._per_voxel(fa_index, nvox, torch.float64, "fa_index", order)
        mask = self._per_voxel(mask, nvox, torch.uint8, "mask", order)
        e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
        fsol, reg = e((nvox, self.n_t2)), e((nvox,))
        sig = e((nvox, self.n_te)) if want_sig else None
        lam = e((nvox,)) if want_lambda else None
        maps = e((6, nvox)) if want_maps else None
        status = e((nvox,), torch.int32) if want_status else None
        sigma_out, flag = e((nvox,)), e((nvox,), torch.int32)
        with torch.cuda.device(dev):
            check(lib().met2_fit_rician(self._h, METHODS[method], nvox, _ptr(data), vs, es, _ptr(fa_index), _ptr(mask), _ptr(sigma), n_iter, _ptr(fsol),
                                        _ptr(sig), _ptr(reg), _ptr(lam), _ptr(maps), _ptr(status), _ptr(sigma_out), _ptr(flag), self._stream()))
        res = {"fsol": fsol, "sig": sig, "reg": reg, "lam": lam, "maps": maps, "status": status, "sigma": sigma_out, "rician_flag": flag}
        if len(vol) > 1:
            res = {k: (None if t is None else unflatten(t, vol, order, lead=1 if k == "maps" else 0)) for k, t in res.items()}
        return res

    def bootstrap_replicates(self, center, sigma, n_rep, seed=0, voxel_id=None):
        """The replicates fit_bootstrap fits (met2_bootstrap_replicates): center [nvox, n_te] and sigma [nvox] float64 CUDA tensors,
        voxel_id [nvox] int64 (default 0..nvox-1) -> [nvox, n_rep, n_te].  No gating: every voxel gets replicates."""
        self._check_data(center, "center")
        self._check_data(sigma, "sigma")
        center = center.contiguous()
        if center.dim() != 2 or center.shape[1] != self.n_te:
            raise ValueError("center must be [nvox, n_te=%d]" % self.n_te)
        nvox = center.shape[0]
        sigma = self._per_voxel(sigma, nvox, torch.float64, "sigma")
        vid = None if voxel_id is None else self._per_voxel(voxel_id, nvox, torch.int64, "voxel_id")
        seed = int(seed)
        if seed >= 2 ** 63:
            seed -= 2 ** 64
        out = torch.empty((nvox, int(n_rep), self.n_te), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().met2_bootstrap_replicates(self._h, nvox, _ptr(center), _ptr(sigma), _ptr(vid), int(n_rep), seed, _ptr(out), self._stream()))
        return out

    @staticmethod
    def _stats_args(t, what, status, nvox):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64:
            raise ValueError("%s must be a float64 CUDA tensor (the hot path has no host fallback)" % what)
        if status is not None:
            status = torch.as_tensor(status, device=t.device)
            if status.numel() != nvox:
                raise ValueError("status has %d entries for %d voxels" % (status.numel(), nvox))
            status = status.reshape(-1).to(torch.int32).contiguous()
        return t.contiguous(), status

    @staticmethod
    def bootstrap_series_stats(values, status=None):
        """The bootstrap's statistics of any series (met2_bootstrap_series_stats; needs no plan): values [n_quant <= 8, nvox, n_rep] or
        [nvox, n_rep] float64 CUDA tensor -> [n_quant, 5, nvox] or [5, nvox] (BOOT_STATS).  status: int per voxel (bit 1 = take it) or None = all;
        the others get zeros.  Finite values and nan; a series with a nan gives five nans."""
        lead = values.dim() == 3 if torch.is_tensor(values) else False
        if not torch.is_tensor(values) or values.dim() not in (2, 3):
            raise ValueError("values must be a [n_quant, nvox, n_rep] or [nvox, n_rep] tensor")
        nq = int(values.shape[0]) if lead else 1
        nvox, n_rep = int(values.shape[-2]), int(values.shape[-1])
        if not 1 <= nq <= 8:
            raise ValueError("n_quant must lie in [1, 8], got %d" % nq)
        if not 2 <= n_rep <= 1024:
            raise ValueError("n_rep must lie in [2, 1024], got %d" % n_rep)
        values, status = Met2Plan._stats_args(values, "values", status, nvox)
        out = torch.empty((nq, 5, nvox), dtype=torch.float64, device=values.device)
        with torch.cuda.device(values.device):
            check(lib().met2_bootstrap_series_stats(values.device.index, nvox, n_rep, nq, _ptr(values), _ptr(status), _ptr(out),
                                                    C.c_void_p(torch.cuda.current_stream(values.device).cuda_stream)))
        return out if lead else out[0]

    @staticmethod
    def bootstrap_spectrum_stats(fsol_r, status=None):
        """The bootstrap's statistics per T2 bin of any replicate spectra (met2_bootstrap_spectrum_stats; needs no plan): fsol_r
        [nvox, n_rep, n_t2] float64 CUDA tensor -> [5, nvox, n_t2] (BOOT_STATS); the same bits as bootstrap_series_stats gives the series
        fsol_r[v, :, j].  status as there."""
        if not torch.is_tensor(fsol_r) or fsol_r.dim() != 3:
            raise ValueError("fsol_r must be a [nvox, n_rep, n_t2] tensor")
        nvox, n_rep, nt2 = (int(x) for x in fsol_r.shape)
        if not 2 <= n_rep <= 1024:
            raise ValueError("n_rep must lie in [2, 1024], got %d" % n_rep)
        if nt2 < 1:
            raise ValueError("n_t2 must be at least 1")
        fsol_r, status = Met2Plan._stats_args(fsol_r, "fsol_r", status, nvox)
        out = torch.empty((5, nvox, nt2), dtype=torch.float64, device=fsol_r.device)
        with torch.cuda.device(fsol_r.device):
            check(lib().met2_bootstrap_spectrum_stats(fsol_r.device.index, nvox, n_rep, nt2, _ptr(fsol_r), _ptr(status), _ptr(out),
                                                      C.c_void_p(torch.cuda.current_stream(fsol_r.device).cuda_stream)))
        return out

    @staticmethod
    def bootstrap_spec_launch_info(n_rep):
        """(T2 bins per tile, doubles between two series of a tile, dynamic LDS in bytes) of the spectrum statistics kernel for n_rep
        replicates (met2_bootstrap_spec_launch_info; host only)."""
        w, S, lds = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        check(lib().met2_bootstrap_spec_launch_info(int(n_rep), C.byref(w), C.byref(S), C.byref(lds)))
        return w.value, S.value, lds.value

    def finish(self):
        """Wait for the current stream and report what fits enqueued with sync=False deferred (met2_plan_finish)."""
        with torch.cuda.device(self.device):
            check(lib().met2_plan_finish(self._h, self._stream()))
        return self

    def objective_grid(self, method, data, lams, fa_index=None):
        """Values of `method`'s lambda-selection objective at `lams` for every voxel -> [nvox, len(lams)].
        The plan's own lambda grid (the L-curve grid) is put back afterwards."""
        lams = np.ascontiguousarray(lams, dtype=np.float64)
        if not 3 <= lams.shape[0] <= min(self.n_t2, 64):
            raise ValueError("objective grid needs 3..min(n_t2, 64) points")
        self._check_data(data)
        data = data.contiguous()
        nvox = data.shape[0]
        fsol = torch.empty((nvox, self.n_t2), dtype=torch.float64, device=data.device)
        reg = torch.empty((nvox,), dtype=torch.float64, device=data.device)
        fa = self._per_voxel(fa_index, nvox, torch.float64, "fa_index")
        saved = self._lam_grid
        self.set_lambda_grid(lams)
        try:
            with torch.cuda.device(data.device):
                check(lib().met2_fit(self._h, 10 + METHODS[method], nvox, _ptr(data), _ptr(fa), _ptr(None), _ptr(fsol), _ptr(None),
                                     _ptr(reg), _ptr(None), _ptr(None), _ptr(None), self._stream()))
                torch.cuda.current_stream(data.device).synchronize()
        finally:
            if saved is not None:
                self.set_lambda_grid(saved)
        return fsol[:, : lams.shape[0]]

    def fa_bruteforce(self, data, mask=None, want_resid=False):
        """fa_estimation.py:74-111 over the plan's flip angles.  data as in fit(); returns flat per-voxel tensors
        (fa_index, km, resid [nvox, n_fa] or None) in the data's voxel order."""
        self._check_data(data)
        data, nvox, vs, es, vol, order = voxel_layout(data, self.n_te)
        dev = self.device
        mask = self._per_voxel(mask, nvox, torch.uint8, "mask", order)
        fa = torch.empty((nvox,), dtype=torch.float64, device=dev)
        km = torch.empty((nvox,), dtype=torch.float64, device=dev)
        resid = torch.empty((nvox, self.n_fa), dtype=torch.float64, device=dev) if want_resid else None
        with torch.cuda.device(dev):
            check(lib().met2_fa_bruteforce_strided(self._h, nvox, _ptr(data), vs, es, _ptr(mask), _ptr(fa), _ptr(km), _ptr(resid), self._stream()))
        return fa, km, resid

    def fa_spline(self, plan_lr, alpha_lr, alpha_hr, data, mask=None, want_xmin=False, want_km=True):
        """Spline FA method (fa_estimation.py:35-70): `plan_lr` holds the coarse-grid dictionary (15 flip angles in the
        driver, motor:237-238), this plan the fine one (273).  Returns (fa_index into alpha_hr, km, xmin or None), flat in
        the data's voxel order."""
        self._check_data(data)
        if plan_lr.device != self.device or plan_lr.n_te != self.n_te:
            raise ValueError("the coarse plan must live on the same device and have the same n_te")
        data, nvox, vs, es, vol, order = voxel_layout(data, self.n_te)
        dev = self.device
        mk = self._per_voxel(mask, nvox, torch.uint8, "mask", order)
        _, _, resid = plan_lr.fa_bruteforce(data, None if mk is None else unflatten(mk, vol, order), want_resid=True)
        (al, pal), (ah, pah) = _h(alpha_lr), _h(alpha_hr)
        fa = torch.empty((nvox,), dtype=torch.float64, device=dev)
        xmin = torch.empty((nvox,), dtype=torch.float64, device=dev) if want_xmin else None
        with torch.cuda.device(dev):
            check(lib().met2_fa_spline_select_strided(dev.index or 0, nvox, al.shape[0], pal, _ptr(resid), ah.shape[0], pah, self.n_te,
                                                      _ptr(data), vs, es, _ptr(mk), _ptr(fa), _ptr(xmin), self._stream()))
        if not want_km:                       # the volume driver never uses it (its Ktotal comes from the final spectra, motor:455-468)
            return fa, None, xmin
        # km = sum of the plain-NNLS spectrum at the selected flip angle (fa_estimation.py:61-64)
        tot = data.sum(dim=-1)
        tot = tot.reshape(-1) if order == "C" else tot.permute(*reversed(range(tot.dim()))).reshape(-1)
        gate = (tot > 0) if mk is None else ((tot > 0) & (mk != 0))
        out = self.fit("NNLS", data, fa_index=fa, mask=gate, want_sig=False, want_maps=False, want_status=False)
        return fa, unflatten_back(out["fsol"], order).sum(dim=1), xmin

    def metrics(self, fsol, mask=None):
        fsol = fsol.contiguous()
        nvox = fsol.shape[0]
        if mask is not None:
            mask = (mask != 0).to(device=fsol.device, dtype=torch.uint8).contiguous()
        maps = torch.empty((6, nvox), dtype=torch.float64, device=fsol.device)
        with torch.cuda.device(fsol.device):
            check(lib().met2_metrics(self._h, nvox, _ptr(fsol), _ptr(mask), _ptr(maps), self._stream()))
        return maps

    def last_kernel_ms(self):
        ms = C.c_double(0.0)
        check(lib().met2_plan_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_second_pass_ms(self):
        ms = C.c_double(0.0)
        check(lib().met2_plan_last_second_pass_ms(self._h, C.byref(ms)))
        return ms.value

    def last_spill_count(self):
        """Voxels of the most recent fit whose passive set outgrew the wave's LDS region and went on in the spill-over slot (under non-default
        lambda-search intervals: every fitted voxel, all of them solved by the spill-over kernel)."""
        n = C.c_int64(0)
        check(lib().met2_plan_last_spill_count(self._h, C.byref(n)))
        return n.value

    def gcv_form(self):
        """(low_rank, residual): whether GCV's trace is taken from the 17 x 17 form in the dictionary's low-rank basis on this plan."""
        lr, res = C.c_int32(0), C.c_double(0.0)
        check(lib().met2_plan_gcv_form(self._h, C.byref(lr), C.byref(res)))
        return bool(lr.value), res.value

    def launch_info(self, method="X2"):
        g, b, l = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(lib().met2_plan_launch_info(self._h, METHODS[method], C.byref(g), C.byref(b), C.byref(l)))
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value}
