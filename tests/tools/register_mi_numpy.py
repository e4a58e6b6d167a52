"""The mutual-information costs of include/met2_hip.h (met2_register_joint_cost), restated in numpy: the samples are register_numpy.sample's
(resample_numpy's order 1: the coordinates, the inside test and the tap indices in fp64), the moving bin of a sample is the header's rule in
fp64 -- it is the contract: scale = moving_bins / (hi - lo) formed once, j = min(max(floor((y - lo) scale), 0), moving_bins - 1), the
subtraction and the product rounded one after the other --, the joint histogram is integers, and the entropies come from the definition
-sum p log p in `dtype` (np.longdouble: the reference the device is held against).  prepare has the signature of register.prepare and serves
as register's cost_fn.  ambiguous names the samples that stand so close to a bin edge that the device's fp64 sample, which agrees with the
long-double one to about 2e-15 and not to the bit, may fall on the other side."""
import numpy as np

import register_numpy as gn

KINDS = ("mi", "nmi")
WORST = {"mi": 0.0, "nmi": -1.0}
EDGE_TOL = 1e-9


def worst(kind):
    return WORST[kind]


def bin_scale(moving_range, moving_bins):
    """-> (lo, scale) in fp64; hi = lo (or a width whose reciprocal overflows) gives scale 0: every sample in bin 0"""
    lo, hi = np.float64(moving_range[0]), np.float64(moving_range[1])
    with np.errstate(over="ignore", divide="ignore"):
        scale = np.float64(moving_bins) / (hi - lo) if hi > lo else np.float64(0.0)
    return lo, (scale if np.isfinite(scale) else np.float64(0.0))


def moving_bin(y, moving_range, moving_bins):
    """the header's rule, in fp64 whatever the dtype of y"""
    lo, scale = bin_scale(moving_range, moving_bins)
    s = (np.asarray(y).astype(np.float64) - lo) * scale
    return np.clip(np.floor(s), 0, moving_bins - 1).astype(np.int64)


def range_of(moving):
    """the range register.prepare passes: the minimum and the maximum of the moving volume"""
    m = np.asarray(moving, dtype=np.float64)
    return float(m.min()), float(m.max())


def joint_of_sample(fixed_bin, moving_range, y, ins, n_bins, moving_bins):
    """-> (n_inside, n_included, joint [n_bins, moving_bins] int64) of one candidate's sample"""
    fixed_bin = np.asarray(fixed_bin)
    included = (fixed_bin >= 0) & (fixed_bin < n_bins)
    use = included & ins
    j = moving_bin(y[use], moving_range, moving_bins)
    joint = np.bincount(fixed_bin[use].astype(np.int64) * moving_bins + j, minlength=n_bins * moving_bins).reshape(n_bins, moving_bins)
    return int(use.sum()), int(included.sum()), joint.astype(np.int64)


def entropy(counts, dtype=np.longdouble):
    """-sum p log p of the non-zero counts, p = count / total"""
    c = np.asarray(counts).reshape(-1)
    p = c[c > 0].astype(dtype) / dtype(c.sum())
    return -(p * np.log(p)).sum()


def cost_of_joint(joint, kind, n_included, min_overlap, dtype=np.longdouble):
    """-> cost of one candidate from its joint histogram; the worst value by the header's integer rules"""
    dtype = np.dtype(dtype).type
    joint = np.asarray(joint, dtype=np.int64)
    n = int(joint.sum())
    if n == 0 or float(n) < float(min_overlap) * float(n_included):
        return worst(kind)
    rows, cols = joint.sum(axis=1), joint.sum(axis=0)
    if (rows == n).any() or (cols == n).any():
        return worst(kind)
    hx, hy, hxy = entropy(rows, dtype), entropy(cols, dtype), entropy(joint, dtype)
    if kind == "mi":
        return float(min(-(hx + hy - hxy), dtype(0)))
    return float(min(-(hx + hy) / hxy, dtype(-1)))


def cost_of_sample(fixed_bin, moving_range, y, ins, kind, n_bins, min_overlap, moving_bins=None, dtype=np.longdouble):
    """-> (n_inside, cost) from the sample of one candidate"""
    mb = n_bins if moving_bins is None else moving_bins
    n, n_incl, joint = joint_of_sample(fixed_bin, moving_range, y, ins, n_bins, mb)
    return n, cost_of_joint(joint, kind, n_incl, min_overlap, dtype)


def ambiguous(fixed_bin, moving_range, y, ins, n_bins, moving_bins):
    """-> (mask [shape] bool, edge [shape] int64): the samples that count and whose scaled value (y - lo) scale, in long double, lies within
    EDGE_TOL of an integer e in 1 .. moving_bins - 1; such a sample may sit in bin e - 1 or in bin e"""
    fixed_bin = np.asarray(fixed_bin)
    lo, scale = bin_scale(moving_range, moving_bins)
    s = (np.asarray(y, dtype=np.longdouble) - np.longdouble(lo)) * np.longdouble(scale)
    e = np.rint(s)
    mask = (fixed_bin >= 0) & (fixed_bin < n_bins) & ins & (np.abs(s - e) <= EDGE_TOL) & (e >= 1) & (e <= moving_bins - 1)
    return mask, np.where(mask, e, 0).astype(np.int64)


def prepare(fixed, fixed_bin, moving, kind="nmi", n_bins=64, min_overlap=0.25, moving_bins=None, dtype=np.longdouble):
    """-> f(A_batch [K, 3, 4]) -> (n_inside [K] int64, cost [K] float64); f(A_batch, want_joint=True) adds joint [K, n_bins, moving_bins]"""
    assert kind in KINDS
    fixed_bin, moving = np.asarray(fixed_bin), np.asarray(moving, dtype=np.float64)
    mb = n_bins if moving_bins is None else moving_bins
    mrange = range_of(moving)
    n_incl = int(((fixed_bin >= 0) & (fixed_bin < n_bins)).sum())

    def evaluate(A_batch, want_joint=False):
        A = np.asarray(A_batch, dtype=np.float64)
        A = A[None] if A.ndim == 2 else A
        ns, cs, js = [], [], []
        for a in A:
            y, ins = gn.sample(moving, a, fixed_bin.shape, dtype)
            n, _, joint = joint_of_sample(fixed_bin, mrange, y, ins, n_bins, mb)
            ns.append(n)
            cs.append(cost_of_joint(joint, kind, n_incl, min_overlap, dtype))
            js.append(joint)
        out = (np.array(ns, dtype=np.int64), np.array(cs, dtype=np.float64))
        return out + (np.stack(js),) if want_joint else out

    return evaluate


def prepare_fp64(fixed, fixed_bin, moving, kind="nmi", n_bins=64, min_overlap=0.25, moving_bins=None):
    """the same with the samples and the entropies in fp64: several times faster, for the searches of the host tests"""
    return prepare(fixed, fixed_bin, moving, kind, n_bins, min_overlap, moving_bins, dtype=np.float64)


# ---------------------------------------------------------------- the end-to-end cases: the remapped phantom of register_numpy

E2E_CASES = {"rigid6_mi": ("rigid6", "mi"), "rigid6_nmi": ("rigid6", "nmi"), "affine12_mi": ("affine12", "mi"), "affine12_nmi": ("affine12", "nmi")}


def e2e_case(name, register_module):
    """-> (true_world, dof, kind, (fixed, fixed_affine, moving, moving_affine, mask)): register_numpy's case with the cost replaced"""
    base, kind = E2E_CASES[name]
    true_world, dof, _, pair = gn.e2e_case(base, register_module)
    return true_world, dof, kind, pair
