"""CPU-only: the numpy restatement of MP-PCA denoising (tests/tools/mppca_numpy.py, the reference of tests/test_gpu_mppca.py) against
known answers, the eigh route against an SVD of the patch matrix, and the seeds the GPU parity tests commit to: on those volumes the
restatement itself must call no voxel a tie.  The ctypes declaration of met2_mppca against the header is covered by
test_host_logic.py, which walks every entry of SYMBOLS."""
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mppca_numpy as mp                                           # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"


def test_library_exports_met2_mppca():
    importlib.import_module(PKG + "._build").build()
    lib = importlib.import_module(PKG + "._lib")
    assert "met2_mppca" in lib.SYMBOLS
    assert hasattr(lib.lib(), "met2_mppca")
    assert lib.lib().met2_abi_version() == 6


def test_eigh_route_matches_svd_route():
    data, mask = mp.two_pool_volume((6, 5, 4), 8, seed=2)
    a = mp.mppca(data, mask, 3, route="eigh")
    b = mp.mppca(data, mask, 3, route="svd")
    assert not mp.ties(a).any()
    assert np.array_equal(a["rank"], b["rank"])
    scale = np.abs(data).max()
    assert np.max(np.abs(a["out"] - b["out"])) <= 1e-11 * scale
    assert np.max(np.abs(a["sigma"] - b["sigma"])) <= 1e-11 * scale
    # N < M (w = 3 patches of at most 27 voxels, 33 echoes): the dropped null space must not leak into either route
    data, mask = mp.two_pool_volume((4, 3, 3), 33, seed=5)
    a = mp.mppca(data, mask, 3, route="eigh")
    b = mp.mppca(data, mask, 3, route="svd")
    assert a["n"].max() <= 27
    assert np.array_equal(a["rank"], b["rank"])
    assert np.max(np.abs(a["out"] - b["out"])) <= 1e-11 * np.abs(data).max()


def test_exact_rank_two_is_found():
    # The rule is a statistical test: with few noise eigenvalues the largest of them now and then passes for signal (at 12 echoes one
    # interior voxel in 27 keeps three components, whichever the seed).  24 echoes against 125 patch voxels leave 22 noise eigenvalues.
    rng = np.random.default_rng(11)
    shape, M = (7, 7, 7), 24
    te = np.arange(1, M + 1)
    basis = np.stack([np.exp(-te / 3.0), np.exp(-te / 9.0)])       # two decay curves: rank 2
    w = 1.0 + rng.random(shape + (2,))                             # signal of order 1: the noise eigenvalues (1e-10) stay above eigh's rounding (1e-13)
    clean = w @ basis
    data = clean + 1e-6 * rng.standard_normal(clean.shape)
    mask = np.ones(shape, dtype=np.uint8)
    res = mp.mppca(data, mask, 5)
    inner = (slice(2, -2),) * 3                                    # full 125-voxel patches
    assert (res["n"][inner] == 125).all()
    assert (res["rank"][inner] == 2).all()
    assert np.max(np.abs(res["out"][inner] - data[inner])) < 1e-4
    assert np.all(res["sigma"][inner] < 1e-5) and np.all(res["sigma"][inner] > 1e-7)


def test_special_cases():
    rng = np.random.default_rng(3)
    data = 10.0 + rng.random((5, 5, 5, 6))
    # a single-voxel mask: N = 1, copied through with rank 1
    mask = np.zeros((5, 5, 5), dtype=np.uint8)
    mask[2, 3, 1] = 1
    res = mp.mppca(data, mask, 3)
    assert np.array_equal(res["out"][2, 3, 1], data[2, 3, 1]) and res["rank"][2, 3, 1] == 1 and res["sigma"][2, 3, 1] == 0.0
    assert res["rank"].sum() == 1 and not res["out"][mask == 0].any()
    # an all-zero patch gives zeros and sigma 0
    mask = np.ones((5, 5, 5), dtype=np.uint8)
    zero = data.copy()
    zero[:3, :3, :3] = 0.0
    res = mp.mppca(zero, mask, 3)
    assert not res["out"][1, 1, 1].any() and res["sigma"][1, 1, 1] == 0.0
    # a nan: exactly the voxels whose patch holds it are copied through with rank -1
    bad = data.copy()
    bad[4, 4, 4, 2] = np.nan
    res = mp.mppca(bad, mask, 3)
    hit = np.zeros((5, 5, 5), dtype=bool)
    hit[3:, 3:, 3:] = True
    assert np.array_equal(res["rank"] == -1, hit)
    assert np.array_equal(res["out"][hit], bad[hit], equal_nan=True) and not res["sigma"][hit].any()
    with pytest.raises(ValueError):
        mp.mppca(data, mask, 4)


@pytest.mark.parametrize("name", sorted(mp.CASES))
def test_committed_seeds_hold_no_ties(name):
    # tests/test_gpu_mppca.py compares the kernel with the restatement on these volumes and may leave out only voxels the restatement calls a
    # tie; the inputs are chosen so that it calls none
    data, mask, w = mp.case(name)
    res = mp.mppca(data, mask, w)
    assert not mp.ties(res).any(), (res["margin"].min(), res["gap"].min())
