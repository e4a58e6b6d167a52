"""GPU tests of the MP-PCA kernel (csrc/met2_mppca.hip) stage by stage, through met2_mppca_stages: the kernel of met2_mppca instantiated a
second time, which copies out the patch list, the Gram matrix, the eigen-solver's result and its sweep count.  Each stage is judged on the
device's own output of the stage before it, so no comparison needs a tie exclusion.

A matrix case (tests/tools/mppca_numpy.py: matrix_case) is a cube whose centre voxel's patch is the whole cube, so that the centre's C is a
matrix the test chose: two-pool data at the echo counts at which the number of pairs rotated side by side or the tournament's shape changes,
and spectra no two-pool volume has (equal, null, clustered, graded, pure noise, zero).

Bounds.
  patch      exact.
  gram       symmetric to the bit; |gram - C_ld| <= N 2^-53 (|X| |X|^T) elementwise, C_ld = X X^T in long double: the dot-product bound.
  eigen      four figures relative to ||C||_2 (mppca_numpy.eig_figures), each at most 50 times the same figure of np.linalg.eigh on the same
             matrix, floored at M 2^-52 (mppca_numpy.eig_bounds; tests/test_mppca_host.py shows eigh's figures).  The margin allows for
             Jacobi applying some hundreds of rotations per column where LAPACK applies O(M) reflectors.  1 <= sweeps <= 30.
  threshold  rank equal and sigma bit-equal to the loop of include/met2_hip.h on the device's eigenvalues: every operation is an IEEE fp64
             add, divide or square root in the stated order.
  projection |out - ref| <= 4 M 2^-53 (|V_s| |V_s|^T |x|) elementwise, ref = V_s (V_s^T x) in long double on the device's eigenvectors: two
             dot products of length M.
With MET2_MPPCA_PARITY_JSON set the measured figures are kept in that file (profiles/mppca_parity.json)."""
import functools
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mppca_numpy as mp                                           # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
L = np.longdouble
NAMES = mp.matrix_case_names()


def record(name, figures):
    """with MET2_MPPCA_PARITY_JSON set, the measured figures are kept in that file (profiles/mppca_parity.json was written this way)"""
    path = os.environ.get("MET2_MPPCA_PARITY_JSON")
    if not path:
        return
    table = json.load(open(path)) if os.path.exists(path) else {}
    table[name] = figures
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def stages():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".mppca").mppca_stages


@functools.lru_cache(maxsize=None)
def staged(name, kind="matrix"):
    """(data, mask, window, the stages' result) of a matrix case or of a committed volume: run once, shared, never written to"""
    data, mask, w = mp.matrix_case(name) if kind == "matrix" else (holes_cube() if name == "w7holes" else mp.case(name))
    res = importlib.import_module(PKG + ".mppca").mppca_stages(data, mask, window=w)
    for a in (data, mask) + tuple(res.values()):
        a.setflags(write=False)
    return data, mask, w, res


def holes_cube():
    """a (7,7,7) cube at window 7 with about 20 holes: patch lists of up to 343 entries (more than four ballots), N even and odd"""
    data, mask = mp.two_pool_volume((7, 7, 7), 4, 31, holes=20)
    return data, mask, 7


def flat(res, key):
    a = res[key]
    nvox = int(np.prod(res["rank"].shape))
    return a.reshape((nvox,) + a.shape[3:])


def patch_matrix(data, res, v):
    """X [M, N] of voxel v from the device's own patch list"""
    n = int(flat(res, "n_patch")[v])
    idx = v + flat(res, "patch")[v, :n].astype(np.int64)
    return data.reshape(-1, data.shape[-1])[idx].T


# ---- patch

@pytest.mark.parametrize("name", ["parity", "wide", "tiny", "w7holes"])
def test_patch_list(stages, name):
    data, mask, w, res = staged(name, "volume")
    nx, ny, nz = mask.shape
    counts = []
    for v in range(nx * ny * nz):
        x, y, z = np.unravel_index(v, mask.shape)
        if not mask[x, y, z]:
            assert flat(res, "n_patch")[v] == 0
            continue
        want = mp.patch_indices(mask, x, y, z, w) - v
        counts.append(want.size)
        assert flat(res, "n_patch")[v] == want.size, (x, y, z)
        assert np.array_equal(flat(res, "patch")[v, :want.size], want), (x, y, z)
    counts = np.array(counts)
    print("N from %d to %d" % (counts.min(), counts.max()))
    if name == "w7holes":
        assert counts.max() > 256 and (counts % 2 == 0).any() and (counts % 2 == 1).any()
    if name == "parity":
        assert counts.min() <= 27 < 32 < counts.max() == 125            # fewer and more voxels than echoes


# ---- gram

def check_gram(data, res, v):
    X = patch_matrix(data, res, v)
    N = X.shape[1]
    G = flat(res, "gram")[v]
    assert np.array_equal(G, G.T)
    C_ld = X.astype(L) @ X.astype(L).T
    bound = N * L(2.0) ** -53 * (np.abs(X).astype(L) @ np.abs(X).astype(L).T)
    err = np.abs(G.astype(L) - C_ld)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1)))
    assert np.all(err <= bound), ratio
    return ratio


@pytest.mark.parametrize("name", NAMES)
def test_gram_of_the_centre(stages, name):
    data, mask, w, res = staged(name)
    c = mp.centre(w)
    N = int(flat(res, "n_patch")[c])
    assert N == (2 if name.endswith("_N2") else w ** 3)
    ratio = check_gram(data, res, c)
    print("N = %d: max |gram - C_ld| / bound = %.3f" % (N, ratio))


def test_gram_at_even_and_odd_patch_sizes(stages):
    # every voxel of the cube with holes: N even (the last trip takes two voxels) and odd (the last trip's second voxel is zeroed)
    data, mask, w, res = staged("w7holes", "volume")
    n = flat(res, "n_patch")
    worst = {0: 0.0, 1: 0.0}
    for v in np.flatnonzero(n >= 2):
        worst[int(n[v]) % 2] = max(worst[int(n[v]) % 2], check_gram(data, res, v))
    print("max |gram - C_ld| / bound: even N %.3f, odd N %.3f" % (worst[0], worst[1]))
    assert (n[n >= 2] % 2 == 0).any() and (n[n >= 2] % 2 == 1).any()


# ---- eigensystem

@pytest.mark.parametrize("name", NAMES)
def test_eigensystem_of_the_centre(stages, name):
    data, mask, w, res = staged(name)
    c = mp.centre(w)
    Cm, d, V = flat(res, "gram")[c], flat(res, "eigval")[c], flat(res, "eigvec")[c]
    sweeps = int(flat(res, "sweeps")[c])
    assert flat(res, "rank")[c] >= 0
    bounds, own = mp.eig_bounds(Cm)
    got = mp.eig_figures(Cm, d, V)
    for k in sorted(got):
        print("%-9s device %.3e   eigh %.3e   bound %.3e" % (k, got[k], own[k], bounds[k]))
    print("sweeps", sweeps)
    record(name, {"device": got, "eigh": own, "bound": bounds, "sweeps": sweeps, "M": int(d.size), "N": int(flat(res, "n_patch")[c])})
    for k in got:
        assert got[k] <= bounds[k], k
    assert 1 <= sweeps <= 30
    if name in mp.EQUAL_DIAGONAL:
        M, N, a = mp.EQUAL_DIAGONAL[name]
        assert sweeps == 1
        assert np.array_equal(V, np.eye(M))
        assert np.array_equal(d, np.full(M, (N // M) * a * a))


def test_sweep_counts_are_in_range_everywhere(stages):
    data, mask, w, res = staged("parity", "volume")
    ran = res["rank"] > 0
    s = res["sweeps"][(mask != 0) & (res["n_patch"] >= 2)]
    print("sweeps on parity: %d to %d" % (s.min(), s.max()))
    record("parity_sweeps", {"min": int(s.min()), "max": int(s.max())})
    assert ran.any() and s.min() >= 1 and s.max() <= 30
    assert not res["sweeps"][mask == 0].any()


# ---- threshold and projection: every voxel of the cube that ran the solver (the clipped patches of the others are further cases)

def solved(res):
    return np.flatnonzero((flat(res, "n_patch") >= 2) & (flat(res, "rank") >= 0))


@pytest.mark.parametrize("name", NAMES)
def test_threshold_on_the_device_spectrum(stages, name):
    data, mask, w, res = staged(name)
    n, rank, sigma, ev = flat(res, "n_patch"), flat(res, "rank"), flat(res, "sigma"), flat(res, "eigval")
    vs = solved(res)
    assert mp.centre(w) in vs
    for v in vs:
        k, sig, order, lam = mp.threshold_from_eigval(ev[v], int(n[v]))
        assert rank[v] == k, (v, rank[v], k)
        assert sigma[v] == sig, (v, sigma[v], sig)
    c = mp.centre(w)
    M = ev.shape[1]
    r = min(M, int(n[c]))
    print("centre: rank %d of %d, sigma %.6g" % (rank[c], r, sigma[c]))
    if name == "noise":
        assert rank[c] == 0 and sigma[c] > 0                       # the rule keeps nothing
    if name == "zero":
        assert rank[c] == r and sigma[c] == 0.0                    # s2 < s1 never holds: nothing is cut
    if name in mp.EQUAL_DIAGONAL:                                  # the index tie-break fills the slots: the spectrum is the exact one
        M, N, a = mp.EQUAL_DIAGONAL[name]
        cut, sigma2, _ = mp.threshold(np.full(M, (N // M) * a * a / N), N)
        assert rank[c] == M - cut and sigma[c] == np.sqrt(sigma2)


@pytest.mark.parametrize("name", NAMES)
def test_projection_on_the_device_eigenvectors(stages, name):
    data, mask, w, res = staged(name)
    n, rank, ev, V, out = flat(res, "n_patch"), flat(res, "rank"), flat(res, "eigval"), flat(res, "eigvec"), flat(res, "out")
    M = ev.shape[1]
    xs = data.reshape(-1, M)
    worst = 0.0
    for v in solved(res):
        k, _, order, _ = mp.threshold_from_eigval(ev[v], int(n[v]))
        Vs = V[v][:, order[M - k:]].astype(L)
        x = xs[v].astype(L)
        ref = Vs @ (Vs.T @ x)
        bound = 4 * M * L(2.0) ** -53 * (np.abs(Vs) @ (np.abs(Vs).T @ np.abs(x)))
        err = np.abs(out[v].astype(L) - ref)
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1))))
        assert np.all(err <= bound), (v, k)
    print("max |out - ref| / bound = %.3f" % worst)


# ---- the same code as the filter, and the path where the solver gives up

def test_stages_entry_is_bit_equal_to_the_filter(stages):
    motor = importlib.import_module(PKG + ".motor")
    data, mask, w, res = staged("parity", "volume")
    out, sigma, rank = motor.mppca_filter(data, mask, window=w, return_maps=True)
    assert np.array_equal(out, res["out"]) and np.array_equal(sigma, res["sigma"]) and np.array_equal(rank, res["rank"])
    # CUDA tensors in, tensors out
    t = stages(torch.as_tensor(data, device="cuda"), torch.as_tensor(mask, device="cuda"), window=w)
    assert all(torch.is_tensor(t[k]) and t[k].is_cuda and np.array_equal(t[k].cpu().numpy(), res[k]) for k in res)


def test_solver_gives_up_at_the_sweep_cap(stages):
    data, mask, w, full = staged("parity", "volume")
    one = stages(data, mask, window=w, max_sweeps=1)
    more = full["sweeps"] > 1
    assert more.any() and (full["rank"][more] >= 0).all()
    assert (one["rank"][more] == -2).all() and not one["sigma"][more].any()
    assert np.array_equal(one["out"][more], data[more])
    assert (one["sweeps"][more] == 1).all()
    for k in ("out", "sigma", "rank", "sweeps"):
        assert np.array_equal(one[k][~more], full[k][~more]), k
    lib = importlib.import_module(PKG + "._lib")
    with pytest.raises(lib.Met2Error):
        stages(data, mask, window=w, max_sweeps=0)
    with pytest.raises(lib.Met2Error):
        stages(data, mask, window=w, max_sweeps=31)
