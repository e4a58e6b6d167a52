"""numpy restatement of the cluster mass (include/met2_hip.h: MET2_TFCE_MODE_MASS; multicomponent-t2-toolbox_amd/group.py), independent of
union-find and of atomics: the components of {t >= h} come from scipy.ndimage.label, the sums from an int64 np.add.at.

members         the voxels of a map that join a component: t >= h (which a value that is not a number fails), inside the mask
quantise        q(v) = (int64) rint(min(t, T_CAP) * 2^24), ties to even; the scaling by a power of two is exact; +infinity saturates
transform       one map -> out [nx, ny, nz] float64: (double)(the int64 sum of q over the component) * 2^-24 for a member, 0 elsewhere
spatial         a batch of maps -> (out [K, ...], kmax [K]); modes other than 'mass' go to tfce_numpy.spatial
batch_spatial, batch_spatial_f, batch_spatial_vsm
                randomise's stand-ins for t, F and the pseudo-t that handle 'mass' (and hand the other modes to the existing stand-ins)
flood_mass      brute force for the cross-checks: the flood fill of tfce_numpy, the sums in Python integers, the quantisation by
                fractions.Fraction -- nothing shared with the restatement but the definition
exact_sum       the component sums of the raw doubles in long double: what the bound is measured against"""
import fractions

import numpy as np
from scipy import ndimage

import group_f_numpy as gf
import group_numpy as gn
import group_vsm_numpy as gv
import tfce_numpy as tn

FRAC_BITS, T_CAP, MAX_G = 24, 16384.0, 1 << 24                     # MET2_TFCE_MASS_FRAC_BITS, MET2_TFCE_MASS_T_CAP, MET2_TFCE_MASS_MAX_G
SCALE = float(1 << FRAC_BITS)


def members(t, h, mask=None):
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        m = np.float64(h) <= t
    return m if mask is None else m & (np.asarray(mask) != 0)


def quantise(t):
    """q of every value as if it were a member (the caller masks); np.rint rounds ties to even"""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(t < T_CAP, t, T_CAP)
    return np.rint(c * SCALE).astype(np.int64)


def transform(t, h, mask=None, connectivity=26):
    t = np.asarray(t, dtype=np.float64)
    mem = members(t, h, mask)
    lab, n = ndimage.label(mem, structure=tn.structure(connectivity))
    q = np.where(mem, quantise(np.where(mem, t, 0.0)), 0)
    total = np.zeros(n + 1, dtype=np.int64)
    np.add.at(total, lab.ravel(), q.ravel())
    return np.where(mem, total[lab].astype(np.float64) * (1.0 / SCALE), 0.0)      # int64 -> float64 rounds to nearest even, once


def spatial(maps, mask=None, mode="mass", dh=1.0, E=0.5, H=2.0, connectivity=26, dtype=np.float64):
    if mode != "mass":
        return tn.spatial(maps, mask, mode, dh, E, H, connectivity, dtype)
    maps = np.asarray(maps, dtype=np.float64)
    out = np.stack([transform(m, dh, mask, connectivity) for m in maps]) if len(maps) else np.empty(maps.shape)
    return out, out.reshape(len(maps), -1).max(axis=1)


def _entry(stat, grid, at, mode, dh, E, H, connectivity, ref, want_first):
    """the group entries' outputs from the statistic [K, V]"""
    maps, mask = tn.dense(np.asarray(stat, dtype=np.float64), grid, at)
    out, _ = spatial(maps, mask, mode, dh, E, H, connectivity)
    s = out.reshape(out.shape[0], -1)[:, at]
    count = None if ref is None else (s >= np.asarray(ref, dtype=np.float64)[None, :]).sum(axis=0).astype(np.uint32)
    return s.max(axis=1), count, (s[0].copy() if want_first else None)


def batch_spatial(Y, s0, W, grid, at, mode, dh, E, H, connectivity, ref, want_first):
    """randomise's batch_spatial on t (met2_group_perm_tfce)"""
    if mode != "mass":
        return tn.batch_spatial(Y, s0, W, grid, at, mode, dh, E, H, connectivity, ref, want_first)
    return _entry(gn.perm_t(Y, s0, W, False, np.float64)[0], grid, at, mode, dh, E, H, connectivity, ref, want_first)


def batch_spatial_f(Y, s0, W, s, scale, grid, at, mode, dh, E, H, connectivity, ref, want_first):
    """randomise's batch_spatial on F (met2_group_perm_ftfce)"""
    if mode != "mass":
        return gf.batch_spatial(Y, s0, W, s, scale, grid, at, mode, dh, E, H, connectivity, ref, want_first)
    return _entry(gf.perm_f(Y, s0, W, s, scale, np.float64)[0], grid, at, mode, dh, E, H, connectivity, ref, want_first)


def batch_spatial_vsm(Y, s0, W, grid, at, mode, dh, E, H, connectivity, ref, want_first, two_sided, radius, taps):
    """randomise's batch_spatial on the pseudo-t (met2_group_perm_vsm)"""
    if mode != "mass":
        return gv.batch_spatial(Y, s0, W, grid, at, mode, dh, E, H, connectivity, ref, want_first, two_sided, radius, taps)
    assert not two_sided and tuple(radius) == tuple((len(t) - 1) // 2 for t in taps)
    return _entry(gv.perm_vt(Y, s0, W, grid, at, taps, False, np.float64), grid, at, mode, dh, E, H, connectivity, ref, want_first)


# ---------------------------------------------------------------- brute force, for the restatement's own cross-checks

def _components(member, connectivity):
    """lists of (x, y, z) by tfce_numpy's stack-based flood fill over explicit neighbours"""
    member = np.asarray(member, dtype=bool)
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if 0 < abs(dx) + abs(dy) + abs(dz) <= reach]
    seen, comps = np.zeros(member.shape, dtype=bool), []
    for start in np.ndindex(member.shape):
        if not member[start] or seen[start]:
            continue
        stack, comp = [start], []
        seen[start] = True
        while stack:
            p = stack.pop()
            comp.append(p)
            for o in offs:
                q = (p[0] + o[0], p[1] + o[1], p[2] + o[2])
                if all(0 <= q[a] < member.shape[a] for a in range(3)) and member[q] and not seen[q]:
                    seen[q] = True
                    stack.append(q)
        comps.append(comp)
    return comps


def _q_exact(x):
    """q of one member's value in exact rational arithmetic: the nearest integer to min(x, cap) 2^24, a tie to the even one"""
    x = float(x)
    f = fractions.Fraction(T_CAP if x > T_CAP else x) * (1 << FRAC_BITS)         # Fraction(float) is exact; +infinity never gets here
    lo = f.numerator // f.denominator
    rest = f - lo
    half = fractions.Fraction(1, 2)
    return lo + (1 if rest > half or (rest == half and lo % 2) else 0)


def flood_mass(t, h, mask=None, connectivity=26):
    """the mass of every member's component: flood fill, Python integers, one correctly rounded conversion (int / int division of Python
    integers is correctly rounded)"""
    t = np.asarray(t, dtype=np.float64)
    mem = np.zeros(t.shape, dtype=bool)
    for idx in np.ndindex(t.shape):
        mem[idx] = (mask is None or bool(mask[idx])) and bool(t[idx] >= h)
    out = np.zeros(t.shape)
    for comp in _components(mem, connectivity):
        total = sum(_q_exact(T_CAP if np.isposinf(t[p]) else t[p]) for p in comp)
        for p in comp:
            out[p] = total / (1 << FRAC_BITS)
    return out


def exact_sum(t, h, mask=None, connectivity=26):
    """-> (the long double sum of the raw t over every member's component, the component's size e), 0 off the members"""
    t = np.asarray(t, dtype=np.float64)
    mem = members(t, h, mask)
    lab, n = ndimage.label(mem, structure=tn.structure(connectivity))
    total = np.zeros(n + 1, dtype=np.longdouble)
    np.add.at(total, lab.ravel(), np.where(mem, t, 0.0).astype(np.longdouble).ravel())
    size = np.bincount(lab.ravel(), minlength=n + 1)
    return np.where(mem, total[lab], 0), np.where(mem, size[lab], 0)
