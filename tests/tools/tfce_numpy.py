"""numpy restatements of the spatial statistics (include/met2_hip.h: met2_tfce, met2_group_perm_tfce; multicomponent-t2-toolbox_amd/group.py),
independent of union-find: per level the components come from scipy.ndimage.label, their sizes from np.bincount.

levels          level(v): the largest j in 1 .. max_steps with j * dh <= t(v), by comparisons (searchsorted over the table of h_j); 0 outside
                the mask and where t is not a number
transform       one map: out and the components' count per level, in any dtype: float64 gives the entry's bits for E = 0.5, H = 2 (a term is
                sqrt(e) * (h * h), the sum runs j = level(v) .. 1 from 0.0, out = dh * sum) and for the extent; long double is the accuracy
                reference for other exponents (a term is e ** E * h ** H)
spatial         a batch of maps -> (out [K, ...], kmax [K])
batch_spatial   met2_group_perm_tfce in float64 with randomise's batch_spatial signature, on group_numpy's t: the host stand-in for the entry
flood_levels, flood_sizes
                brute force that uses neither searchsorted nor ndimage: for the cross-checks of the restatement itself
planted_case, planted_host
                the case the host and the device tests share, and its run on the host"""
import numpy as np
from scipy import ndimage

import group_numpy as gn

LD = np.longdouble
MAX_STEPS = 1024


def structure(connectivity):
    """the 3 x 3 x 3 neighbourhood of connectivity 6 (faces), 18 (and edges) or 26 (and corners)"""
    return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])


def levels(t, dh, mask=None, max_steps=MAX_STEPS):
    t = np.asarray(t, dtype=np.float64)
    h = np.arange(1, max_steps + 1, dtype=np.float64) * np.float64(dh)     # h_j, one rounding each
    lev = np.searchsorted(h, np.where(np.isnan(t), -np.inf, t), side="right")       # the number of h_j <= t: comparisons only
    if mask is not None:
        lev = np.where(np.asarray(mask) != 0, lev, 0)
    return lev.astype(np.int64)


def transform(t, mask=None, mode="tfce", dh=1.0, E=0.5, H=2.0, connectivity=6, dtype=np.float64, max_steps=MAX_STEPS):
    """-> (out [nx, ny, nz] in dtype, n_components [top + 1]: the number of components of S_j, entry 0 unused)"""
    t = np.asarray(t, dtype=np.float64)
    lev = levels(t, dh, mask, 1 if mode == "extent" else max_steps)
    top = int(lev.max(initial=0))
    acc = np.zeros(t.shape, dtype=dtype)
    ncomp = np.zeros(top + 1, dtype=np.int64)
    st = structure(connectivity)
    half_two = E == 0.5 and H == 2.0
    for j in range(top, 0, -1):
        lab, ncomp[j] = ndimage.label(lev >= j, structure=st)
        e = np.bincount(lab.ravel())[lab].astype(dtype)            # every voxel's component size (label 0: not in S_j, masked below)
        if mode == "extent":
            term = e
        else:
            h = dtype(np.float64(j) * np.float64(dh))              # h_j is the float64 product in every dtype: it defines the level
            term = np.sqrt(e) * (h * h) if half_two else e ** dtype(E) * h ** dtype(H)
        acc = np.where(lab > 0, acc + term, acc)
    return (acc if mode == "extent" else dtype(np.float64(dh)) * acc), ncomp


def spatial(maps, mask=None, mode="tfce", dh=1.0, E=0.5, H=2.0, connectivity=6, dtype=np.float64):
    maps = np.asarray(maps, dtype=np.float64)
    out = np.stack([transform(m, mask, mode, dh, E, H, connectivity, dtype)[0] for m in maps]) if len(maps) else np.empty(maps.shape, dtype=dtype)
    return out, out.reshape(len(maps), -1).max(axis=1)


def dense(t, grid, at):
    """t [K, V] on the grid -> (maps [K, nx, ny, nz] with 0 elsewhere, mask [nx, ny, nz])"""
    G = int(np.prod(grid))
    maps, mask = np.zeros((t.shape[0], G)), np.zeros(G, dtype=np.uint8)
    maps[:, at] = t
    mask[at] = 1
    return maps.reshape((t.shape[0],) + tuple(grid)), mask.reshape(grid)


def perm_spatial(Y, s0, W, grid, at, mode, dh, E, H, connectivity, ref=None, dtype=np.float64):
    """-> dict(s [K, V], kmax [K], count [V] uint32 or None): the group entry's outputs from the float64 t of group_numpy"""
    t = gn.perm_t(Y, s0, W, False, np.float64)[0]
    maps, mask = dense(t, grid, at)
    out, _ = spatial(maps, mask, mode, dh, E, H, connectivity, dtype)
    s = out.reshape(out.shape[0], -1)[:, at]
    count = None if ref is None else (s >= np.asarray(ref, dtype=dtype)[None, :]).sum(axis=0).astype(np.uint32)
    return {"s": s, "kmax": s.max(axis=1), "count": count}


def batch_spatial(Y, s0, W, grid, at, mode, dh, E, H, connectivity, ref, want_first):
    """randomise's batch_spatial: the entry in float64 -> (kmax, count increment or None, first or None)"""
    r = perm_spatial(Y, s0, W, grid, at, mode, dh, E, H, connectivity, ref)
    return r["kmax"], r["count"], (r["s"][0].copy() if want_first else None)


# ---------------------------------------------------------------- brute force, for the restatement's own cross-checks

def flood_levels(t, dh, mask=None, max_steps=MAX_STEPS):
    """level(v) by counting upward one threshold at a time"""
    t = np.asarray(t, dtype=np.float64)
    lev = np.zeros(t.shape, dtype=np.int64)
    for idx in np.ndindex(t.shape):
        if mask is not None and not mask[idx]:
            continue
        j = 0
        while j < max_steps and np.float64(j + 1) * np.float64(dh) <= t[idx]:
            j += 1
        lev[idx] = j
    return lev


def flood_sizes(member, connectivity):
    """every member's component size by a stack-based flood fill over explicit (x, y, z) neighbours"""
    member = np.asarray(member, dtype=bool)
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if 0 < abs(dx) + abs(dy) + abs(dz) <= reach]
    size, seen = np.zeros(member.shape, dtype=np.int64), np.zeros(member.shape, dtype=bool)
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
        for p in comp:
            size[p] = len(comp)
    return size


def flood_tfce(t, mask, dh, connectivity, max_steps=MAX_STEPS):
    """TFCE with E = 0.5, H = 2 from flood_levels and flood_sizes, in the stated order"""
    lev = flood_levels(t, dh, mask, max_steps)
    acc = np.zeros(lev.shape)
    for j in range(int(lev.max(initial=0)), 0, -1):
        e = flood_sizes(lev >= j, connectivity).astype(np.float64)
        h = np.float64(j) * np.float64(dh)
        acc = np.where(lev >= j, acc + np.sqrt(e) * (h * h), acc)
    return np.float64(dh) * acc


# ---------------------------------------------------------------- the case the host and the device tests share

PLANTED_GRID, PLANTED_BLOCK = (16, 16, 8), (slice(5, 11), slice(5, 11), slice(2, 6))


def planted_case(n=12, shift=1.1, seed=3):
    """one-sample data on a 16 x 16 x 8 grid, every voxel tested: unit normal noise, +shift sigma in a 6 x 6 x 4 block
    -> (Y [n, V], X, c, grid, at [V], block [V] bool, near [V] bool: the block grown by one voxel (26 neighbours))"""
    grid = PLANTED_GRID
    V = int(np.prod(grid))
    block = np.zeros(grid, dtype=bool)
    block[PLANTED_BLOCK] = True
    Y = np.random.default_rng(seed).standard_normal((n, V))
    Y[:, block.ravel()] += shift
    X, c = gn.one_sample_design(n)
    near = ndimage.binary_dilation(block, structure=structure(26))
    return Y, X, c, grid, np.arange(V), block.ravel(), near.ravel()


_PLANTED = {}


def planted_host(group):
    """the planted case through group.randomise with the restatements as batch_stat and batch_spatial (400 sign flips, TFCE with the defaults and
    the cluster extent at 2.5), computed once -> (Y, X, c, grid, at, block, near, out)"""
    if not _PLANTED:
        Y, X, c, grid, at, block, near = planted_case()
        out = group.randomise(Y, X, c, n_perm=400, seed=0, exchange="flip", batch_stat=gn.batch_stat, batch_spatial=batch_spatial, tfce=True,
                              cluster_threshold=2.5, grid=grid, at=at)
        _PLANTED["run"] = (Y, X, c, grid, at, block, near, out)
    return _PLANTED["run"]
