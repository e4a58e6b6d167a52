"""Monte-Carlo accuracy study of the fit methods: the GPU counterpart of the reference's
scripts_synthetic_data_evaluation/Paper_Comparison/evaluate_all_methods_two_lobes_SNR{50_150,150_300,_Inf}.py.

    res = evaluate_methods(n_voxels=10000, snr=(50, 150), seed=0)
    res.errors            # [10, 13]  the columns of table_errors.txt
    res.regularization    # [10, 2]   mean and std of the selected lambda (table_regularization.txt)
    res.write_tables(out) # table_errors.{txt,csv}, table_regularization.{txt,csv} in the reference's layout

Every numeric step runs in libmet2_hip.so: the generator (met2_synth_two_lobe), the flip-angle search and fits (the plan's),
the per-voxel metrics (met2_eval_voxel_metrics) and the aggregates (met2_eval_reduce).  torch holds device memory only."""
import ctypes as C
import math
import os

import numpy as np
import torch

from ._lib import SynthParams, check, lib
from .plan import Met2Plan, _ptr

PAPER_METHODS = ("1. NNLS", "2. X2-I", "3. X2-L1", "4. X2-L2", "5. Lcurve-I", "6. Lcurve-L1", "7. Lcurve-L2", "8. GCV-I", "9. GCV-L1",
                 "10. GCV-L2")
# the reference's calls (:438-576): reg_method and penalty order of create_Laplacian_matrix
METHOD_SPEC = {"1. NNLS": ("NNLS", "I"), "2. X2-I": ("X2", "I"), "3. X2-L1": ("X2", "L1"), "4. X2-L2": ("X2", "L2"),
               "5. Lcurve-I": ("L_curve", "I"), "6. Lcurve-L1": ("L_curve", "L1"), "7. Lcurve-L2": ("L_curve", "L2"),
               "8. GCV-I": ("GCV", "I"), "9. GCV-L1": ("GCV", "L1"), "10. GCV-L2": ("GCV", "L2")}
ERROR_COLUMNS = ("1. MAE", "2. MARE", "3. RMSE", "4. cRMSE", "5. RMSRE", "6. U95", "7. MBE", "8. R", "9. GMARE", "10. MAE-k", "11. MAE-S",
                 "12. MJSD-S", "13. MWD-S")
REG_COLUMNS = ("mean Lambda", "STD")
# met2_eval_voxel_metrics' rows and met2_synth_two_lobe's truth rows (include/met2_hip.h)
FIELDS = ("fM", "fIE", "T2m", "T2IE", "km", "npeaks", "mae_s", "jsd", "wd")
TRUTH = ("MWF", "T2m", "T2ie", "Km", "FA", "SNR", "MWF_draw", "sigma_m", "sigma_ie")
# the reference's ranges (:156-170)
RANGES = {"mwf": (0.05, 0.25), "t2m": (15.0, 35.0), "t2ie": (60.0, 90.0), "fa": (90.0, 180.0), "sm": (1.0, 3.0), "sie": (6.0, 12.0)}
# L-curve at more than 64 bins is fitted in slices of this many voxels: within the spill-over kernel's record cap, so that the outcome
# does not depend on the chunk size (met2_fit_bootstrap uses the same bound)
_LCURVE_SLICE = 4096


def study_t2_grid(npc=60):
    # :192-198
    return np.logspace(math.log10(10.0), math.log10(2000.0), num=npc, endpoint=True, base=10.0)


def study_lambda_grid(num=50):
    # :213-215: 0 and logspace(1e-8, 100, 49) -- the study's grid, not the driver's (which tops at 10)
    lam = np.zeros(num)
    lam[1:] = np.logspace(math.log10(1e-8), math.log10(100.0), num=num - 1, endpoint=True, base=10.0)
    return lam


def synth_params(snr=(50.0, 150.0), te=10.0, TR=3000.0, T1=1000.0, km=1000.0, **ranges):
    """met2_synth_params for an SNR band (lo, hi), or snr=None for the noise-free band.  ranges: mwf, t2m, t2ie, fa, sm, sie = (lo, hi)."""
    p = SynthParams()
    p.struct_size = C.sizeof(SynthParams)
    p.te, p.TR, p.T1, p.km = float(te), float(TR), float(T1), float(km)
    r = dict(RANGES)
    for k, v in ranges.items():
        if k not in r:
            raise ValueError("unknown range %r (have %s)" % (k, sorted(r)))
        r[k] = v
    for k, (lo, hi) in r.items():
        setattr(p, k + "_lo", float(lo)); setattr(p, k + "_hi", float(hi))
    if snr is None:
        p.snr_lo = p.snr_hi = math.inf
    else:
        p.snr_lo, p.snr_hi = float(snr[0]), float(snr[1])
    return p


def _seed64(seed):
    seed = int(seed)
    if not -2 ** 63 <= seed < 2 ** 64:
        raise ValueError("seed must fit in 64 bits")
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


def synth_two_lobe(plan, n, seed=0, snr=(50.0, 150.0), voxel_offset=0, te=10.0, TR=3000.0, T1=1000.0, km=1000.0, **ranges):
    """n two-lobe voxels by the reference's recipe on `plan`'s device, T2 grid and myelin cut-off.  Voxel v is the study's voxel
    voxel_offset + v: its draws depend on (seed, voxel_offset + v) alone.  Returns a dict of float64 device tensors: data [n, n_te],
    dist2 [n, n_t2] (the true low-resolution spectrum) and truth [9, n] (rows TRUTH)."""
    n = int(n)
    if n < 0 or voxel_offset < 0:
        raise ValueError("n and voxel_offset must be >= 0")
    p = synth_params(snr, te, TR, T1, km, **ranges)
    dev = plan.device
    data = torch.empty((n, plan.n_te), dtype=torch.float64, device=dev)
    dist2 = torch.empty((n, plan.n_t2), dtype=torch.float64, device=dev)
    truth = torch.empty((len(TRUTH), n), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().met2_synth_two_lobe(plan._h, C.byref(p), n, _seed64(seed), int(voxel_offset), _ptr(data), _ptr(dist2), _ptr(truth),
                                        plan._stream()))
    return {"data": data, "dist2": dist2, "truth": truth}


def voxel_metrics(plan, fsol, dist2):
    """estimate_error_metrics (:59-74) per voxel -> [9, n] device tensor (rows FIELDS)."""
    fsol, dist2 = fsol.contiguous(), dist2.contiguous()
    n = fsol.shape[0]
    out = torch.empty((len(FIELDS), n), dtype=torch.float64, device=fsol.device)
    with torch.cuda.device(fsol.device):
        check(lib().met2_eval_voxel_metrics(plan._h, n, _ptr(fsol), _ptr(dist2), _ptr(out), plan._stream()))
    return out


def reduce_metrics(per_voxel, truth, lam=None, fie=None):
    """compute_multi_metrics (:77-123) and mean / std of lambda -> numpy [15]: ERROR_COLUMNS then REG_COLUMNS.  per_voxel [9, n],
    truth [9, n], lam [n] or None, fie [n] or None (the fIE GMARE reads; None = per_voxel's own) -- device tensors."""
    per_voxel, truth = per_voxel.contiguous(), truth.contiguous()
    n = per_voxel.shape[1]
    out = torch.empty((len(ERROR_COLUMNS) + 2,), dtype=torch.float64, device=per_voxel.device)
    lam = None if lam is None else lam.contiguous()
    fie = None if fie is None else fie.contiguous()
    with torch.cuda.device(per_voxel.device):
        check(lib().met2_eval_reduce(n, _ptr(per_voxel), _ptr(truth), _ptr(lam), _ptr(fie), _ptr(out),
                                     C.c_void_p(torch.cuda.current_stream(per_voxel.device).cuda_stream)))
    return out.cpu().numpy()


def _fmt_g(v):
    return format(float(v), "g")


def _afterpoint(s):
    # tabulate's _afterpoint: digits after the decimal point (or after the exponent mark), -1 for an integer
    try:
        int(s)
        return -1
    except ValueError:
        pass
    pos = s.rfind(".")
    pos = s.lower().rfind("e") if pos < 0 else pos
    return len(s) - pos - 1 if pos >= 0 else -1


def format_table(headers, rows):
    """The layout of tabulate(rows, headers) with its defaults ('simple' format): text columns stripped and left-aligned, numeric columns
    in format 'g' aligned on the decimal point, headers right-aligned over numeric columns, two spaces between columns."""
    ncol = len(headers)
    cols = []
    for c in range(ncol):
        vals = [r[c] for r in rows]
        if all(isinstance(v, (int, float, np.integer, np.floating)) for v in vals):
            s = [_fmt_g(v) for v in vals]
            dec = [_afterpoint(x) for x in s]
            md = max(dec)
            s = [x + " " * (md - d) for x, d in zip(s, dec)]
            cols.append((s, "right"))
        else:
            cols.append(([str(v).strip() for v in vals], "left"))
    widths = [max([len(headers[c]) + 2] + [len(x) for x in cols[c][0]]) for c in range(ncol)]
    pad = lambda x, w, how: x.ljust(w) if how == "left" else x.rjust(w)
    lines = ["  ".join(pad(headers[c], widths[c], cols[c][1]) for c in range(ncol)).rstrip(),
             "  ".join("-" * w for w in widths).rstrip()]
    for i in range(len(rows)):
        lines.append("  ".join(pad(cols[c][0][i], widths[c], cols[c][1]) for c in range(ncol)).rstrip())
    return "\n".join(lines)


class EvalResult:
    """methods: row labels; errors [rows, 13] (ERROR_COLUMNS); regularization [rows, 2] (REG_COLUMNS); per_voxel: None, or a dict
    label -> dict of numpy arrays (FIELDS and 'lam'), plus 'truth' -> dict (TRUTH) and 'fa_index'."""

    def __init__(self, methods, errors, regularization, per_voxel=None, params=None):
        self.methods = tuple(methods)
        self.errors = np.asarray(errors, dtype=np.float64)
        self.regularization = np.asarray(regularization, dtype=np.float64)
        self.per_voxel = per_voxel
        self.params = params or {}

    def error_table(self):
        return format_table(("Method",) + ERROR_COLUMNS, [[m] + list(r) for m, r in zip(self.methods, self.errors)])

    def _reg_rows(self):
        # the reference writes the NNLS row as the integers 0, 0 (:755)
        return [[m.ljust(22)] + ([0, 0] if m == "1. NNLS" else list(r)) for m, r in zip(self.methods, self.regularization)]

    def regularization_table(self):
        return format_table(("Method                ",) + REG_COLUMNS, self._reg_rows())

    def write_tables(self, out_dir):
        """table_errors.{txt,csv} and table_regularization.{txt,csv} as the reference writes them (:737-772): the .txt through tabulate's
        layout (no trailing newline), the .csv without header, errors at 4 decimals, lambdas at full precision."""
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "table_errors.txt"), "w") as f:
            f.write(self.error_table())
        with open(os.path.join(out_dir, "table_errors.csv"), "w") as f:
            for m, r in zip(self.methods, self.errors):
                f.write(",".join([m] + ["%.4f" % v for v in r]) + "\n")
        with open(os.path.join(out_dir, "table_regularization.txt"), "w") as f:
            f.write(self.regularization_table())
        with open(os.path.join(out_dir, "table_regularization.csv"), "w") as f:
            for r in self._reg_rows():
                f.write(",".join([r[0]] + [repr(v) if isinstance(v, int) else repr(float(v)) for v in r[1:]]) + "\n")
        return out_dir


def evaluate_methods(n_voxels=10000, snr=(50.0, 150.0), seed=0, nte=32, te=10.0, npc=60, TR=3000.0, methods=PAPER_METHODS, lambda_grid=None,
                     chunk=65536, per_voxel=False, device=0, x2_factor=1.02, gmare_fie="nnls", rician=None, rician_iters=3):
    """The reference's study (evaluate_all_methods_two_lobes_SNR*.py) for one SNR band: snr=(lo, hi), or None for the noise-free band.
    Per chunk of voxels on one plan (nte x npc x 91 flip angles): generate; brute-force flip angle over the 91-angle dictionary on the
    noisy, unnormalised signal (:398); fit every method (lambda from the fit's `lam`, :469); per-voxel metrics.  Then one reduction per
    method over all voxels.  gmare_fie='nnls' is the reference's GMARE: its fIE term reads the NNLS fit for every method (:107); 'own'
    reads each method's.  Results do not depend on `chunk`.  rician='iterative' (an extension): every method's fit goes through
    Met2Plan.fit_rician with rician_iters passes, the noise level estimated per voxel (Met2Plan.noise_sigma), not taken from the truth; the
    tables keep their layout."""
    methods = tuple(methods)
    if rician not in (None, "iterative"):
        raise ValueError("rician must be None or 'iterative'")
    if not 0 <= int(rician_iters) <= 16:
        raise ValueError("rician_iters must lie in [0, 16]")
    for m in methods:
        if m not in METHOD_SPEC:
            raise ValueError("unknown method %r (have %s)" % (m, PAPER_METHODS))
    if gmare_fie not in ("nnls", "own"):
        raise ValueError("gmare_fie must be 'nnls' or 'own'")
    n_voxels, chunk = int(n_voxels), int(chunk)
    if n_voxels <= 0 or chunk <= 0:
        raise ValueError("n_voxels and chunk must be positive")
    fitted = methods + (("1. NNLS",) if gmare_fie == "nnls" and "1. NNLS" not in methods else ())
    T2s = study_t2_grid(npc)
    T1s = 1000.0 * np.ones_like(T2s)
    alphas = np.linspace(90.0, 180.0, 91)
    plan = Met2Plan(nte, npc, alphas.shape[0], device=device, x2_factor=x2_factor)
    try:
        plan.build_dictionary_epg(T2s, T1s, te, alphas, TR)
        plan.set_lambda_grid(study_lambda_grid() if lambda_grid is None else lambda_grid)
        dev = plan.device
        pv = {m: torch.empty((len(FIELDS), n_voxels), dtype=torch.float64, device=dev) for m in fitted}
        lam = {m: torch.zeros((n_voxels,), dtype=torch.float64, device=dev) for m in fitted}
        truth = torch.empty((len(TRUTH), n_voxels), dtype=torch.float64, device=dev)
        fa_all = torch.empty((n_voxels,), dtype=torch.float64, device=dev)
        pen = None
        for s in range(0, n_voxels, chunk):
            e = min(n_voxels, s + chunk)
            g = synth_two_lobe(plan, e - s, seed=seed, snr=snr, voxel_offset=s, te=te, TR=TR)
            truth[:, s:e] = g["truth"]
            fa, _, _ = plan.fa_bruteforce(g["data"])
            fa_all[s:e] = fa
            for m in fitted:
                method, p = METHOD_SPEC[m]
                if p != pen:
                    plan.set_penalty(p)
                    pen = p
                step = _LCURVE_SLICE if method == "L_curve" and npc > 64 else e - s
                for a in range(0, e - s, step):
                    b = min(e - s, a + step)
                    if rician:
                        out = plan.fit_rician(method, g["data"][a:b], n_iter=int(rician_iters), fa_index=fa[a:b], want_sig=False, want_maps=False,
                                              want_status=False, want_lambda=method != "NNLS")
                    else:
                        out = plan.fit(method, g["data"][a:b], fa_index=fa[a:b], want_sig=False, want_maps=False, want_status=False,
                                       want_lambda=method != "NNLS")
                    pv[m][:, s + a:s + b] = voxel_metrics(plan, out["fsol"], g["dist2"][a:b])
                    if method != "NNLS":
                        lam[m][s + a:s + b] = out["lam"]
        fie = pv["1. NNLS"][1] if gmare_fie == "nnls" else None
        agg = np.stack([reduce_metrics(pv[m], truth, None if METHOD_SPEC[m][0] == "NNLS" else lam[m], fie) for m in methods])
        torch.cuda.synchronize(dev)
        pvd = None
        if per_voxel:
            pvd = {m: dict({f: pv[m][i].cpu().numpy() for i, f in enumerate(FIELDS)}, lam=lam[m].cpu().numpy()) for m in fitted}
            pvd["truth"] = {f: truth[i].cpu().numpy() for i, f in enumerate(TRUTH)}
            pvd["fa_index"] = fa_all.cpu().numpy()
        params = dict(n_voxels=n_voxels, snr=snr, seed=seed, nte=nte, te=te, npc=npc, TR=TR, chunk=chunk, gmare_fie=gmare_fie, rician=rician, rician_iters=int(rician_iters))
        return EvalResult(methods, agg[:, :13], agg[:, 13:], pvd, params)
    finally:
        plan.close()
