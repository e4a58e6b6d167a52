"""CPU-only: the numpy restatement of the 3-D Gibbs-ringing removal (tests/tools/gibbs3d_numpy.py, the reference of
tests/test_gpu_gibbs3d.py) against the properties include/met2_hip.h states for met2_degibbs3d, a known answer (a ball that rings along all
three axes) and a dense long-double DFT; and the volumes the GPU parity tests commit to: on those the restatement itself must call no sample
a tie, so the GPU test leaves none out."""
import ctypes as C
import importlib
import itertools
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gibbs_numpy as gn                                           # noqa: E402
import gibbs3d_numpy as g3                                         # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"
SHAPES = ((8, 12, 10), (9, 15, 11), (16, 9, 10), (9, 8, 11), (8, 8, 8))       # three even axes, none, two, one, three


def test_library_exports_the_3d_entries_as_the_header_declares_them():
    importlib.import_module(PKG + "._build").build()
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    assert L.met2_abi_version() == 6
    with open(os.path.join(ROOT, "include", "met2_hip.h")) as f:
        text = f.read()
    ctype = {"int32_t": C.c_int32, "const double *": C.c_void_p, "double *": C.c_void_p, "int8_t *": C.c_void_p, "void *": C.c_void_p}
    for name, count in (("met2_degibbs3d", 14), ("met2_gibbs_split3d", 10)):
        assert name in lib.SYMBOLS and hasattr(L, name)
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        want = [ctype[re.sub(r"\w+$", "", " ".join(arg.split())).strip()] for arg in m.group(1).split(",")]
        assert len(want) == count
        assert list(getattr(L, name).argtypes) == want


@pytest.mark.parametrize("shape", SHAPES)
def test_weights_are_a_partition_of_one(shape):
    g = g3.split_weights3d(*shape)
    for w in g:
        assert w.shape == shape and (w >= 0.0).all() and (w <= 1.0).all()
    assert np.abs(g[0] + g[1] + g[2] - 1.0).max() <= 4e-16
    nyq = [n // 2 if n % 2 == 0 else None for n in shape]
    if all(k is not None for k in nyq):                              # the corner and the three lines through it
        assert [w[nyq[0], nyq[1], nyq[2]] for w in g] == [1.0 / 3.0] * 3
        assert (g[0][nyq[0], nyq[1], 1], g[1][nyq[0], nyq[1], 1], g[2][nyq[0], nyq[1], 1]) == (0.5, 0.5, 0.0)
        assert (g[0][nyq[0], 1, nyq[2]], g[1][nyq[0], 1, nyq[2]], g[2][nyq[0], 1, nyq[2]]) == (0.5, 0.0, 0.5)
        assert (g[0][1, nyq[1], nyq[2]], g[1][1, nyq[1], nyq[2]], g[2][1, nyq[1], nyq[2]]) == (0.0, 0.5, 0.5)
    if nyq[0] is not None:                                           # one c zero alone: that axis takes everything
        assert g[0][nyq[0], 1, 1] == 1.0 and g[1][nyq[0], 1, 1] == 0.0 and g[2][nyq[0], 1, 1] == 0.0


def test_weights_permute_with_the_axes():
    shape = (8, 9, 12)
    g = g3.split_weights3d(*shape)
    for perm in itertools.permutations(range(3)):
        gp = g3.split_weights3d(*[shape[a] for a in perm])
        for k, a in enumerate(perm):                                 # axis k of the permuted volume is axis a of the original
            assert np.abs(gp[k] - np.transpose(g[a], perm)).max() <= 4e-16, perm        # den is summed in another order: an ulp or two


@pytest.mark.parametrize("shape", SHAPES)
def test_parts_sum_to_the_volume(shape):
    V = 100.0 + 5.0 * np.random.default_rng(7).standard_normal(shape)
    parts = g3.split3d(V)
    dev = np.abs(parts[0] + parts[1] + parts[2] - V).max() / np.abs(V).max()
    print("%s: |Ix + Iy + Iz - V| / max|V| = %.2e" % (shape, dev))
    assert dev <= 1e-12


@pytest.mark.parametrize("shape", ((8, 12, 10), (9, 15, 11), (16, 9, 10), (9, 8, 16)))
def test_split_against_a_dense_long_double_dft(shape):
    V = 100.0 + 5.0 * np.random.default_rng(11).standard_normal(shape)
    got, want = g3.split3d(V), g3.ld_split3d(V)
    for a, (x, y) in enumerate(zip(got, want)):
        dev = float(np.abs(x - y).max() / np.abs(V).max())
        print("%s I%s: %.2e of max|V| (long double is %s)" % (shape, g3.AXES[a], dev, "wider" if gn.LD_IS_WIDER else "float64 here"))
        assert dev <= 1e-13
    assert float(np.abs(want[0] + want[1] + want[2] - V).max() / np.abs(V).max()) <= 1e-13


@pytest.mark.parametrize("name", sorted(g3.CASES))
def test_no_committed_case_holds_a_tie(name):
    data, params, res = g3.reference(name)
    margin = g3.min_margin(res)
    print("%s %s: smallest margin %.1e" % (name, data.shape, margin))
    assert not g3.ties(res).any()
    assert margin >= g3.TIE
    nsh = params[0]
    for a in g3.AXES:
        assert np.abs(res["shift_" + a]).max() >= min(2, nsh)


def test_constant_along_z_leaves_the_z_part_alone():
    S = 100.0 + 5.0 * np.random.default_rng(5).standard_normal((12, 10))
    V = np.repeat(S[:, :, None], 9, axis=2)
    out, sx, sy, sz, mx, my, mz, ix, iy, iz = g3.degibbs3d_volume(V)
    assert not sz.any()
    uz = g3.unring_axis(iz, 2, 20, 1, 3)[0]
    assert np.abs(uz - iz).max() <= 1e-12 * np.abs(V).max()
    assert np.abs(iz - iz[:, :, :1]).max() <= 1e-12 * np.abs(V).max()
    assert np.abs(sx).max() >= 2 and np.abs(sy).max() >= 2


def test_non_finite_echo_is_copied_through():
    data = np.array(g3.case("mixed")[0])
    data[3, 4, 5, 1] = np.nan
    res = g3.degibbs3d(data)
    assert np.array_equal(res["out"][..., 1], data[..., 1], equal_nan=True)
    assert not res["shift_x"][..., 1].any() and not res["shift_z"][..., 1].any()
    clean = g3.reference("mixed")[2]
    assert np.array_equal(res["out"][..., 0], clean["out"][..., 0]) and np.array_equal(res["shift_y"][..., 2], clean["shift_y"][..., 2])


def test_known_answer_ball():
    img, truth, flat = g3.ball_phantom()
    res = g3.ball_reference()
    two = gn.degibbs(img[..., None])["out"][..., 0]
    e0, e2, e3 = g3.rms(img, truth, flat), g3.rms(two, truth, flat), g3.rms(res["out"][..., 0], truth, flat)
    tie_share = float(sum((res["margin_" + a] < g3.TIE).sum() for a in g3.AXES)) / (3 * img.size)
    print("ball: rms error over %d flat voxels: input %.3f, 2-D %.3f, 3-D %.3f (ratios %.2f and %.2f); ties %.4f %%, smallest margin %.1e"
          % (flat.sum(), e0, e2, e3, e3 / e0, e3 / e2, 100 * tie_share, g3.min_margin(res)))
    assert flat.sum() > img.size // 2
    assert e3 <= 0.5 * e0
    assert e3 <= 0.75 * e2
    assert tie_share <= 1e-3
