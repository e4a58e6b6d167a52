"""CPU-only: the numpy restatement of the Gibbs-ringing removal (tests/tools/gibbs_numpy.py, the reference of tests/test_gpu_gibbs.py)
against properties and a known answer, its two routes for the sub-voxel shifts against each other, and the volumes the GPU parity tests
commit to: on those the restatement itself must call no sample a tie, so the GPU test leaves none out."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gibbs_numpy as gn                                           # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"


def test_library_exports_met2_degibbs_as_the_header_declares_it():
    importlib.import_module(PKG + "._build").build()
    lib = importlib.import_module(PKG + "._lib")
    assert "met2_degibbs" in lib.SYMBOLS
    L = lib.lib()
    assert hasattr(L, "met2_degibbs")
    assert L.met2_abi_version() == 6
    with open(os.path.join(ROOT, "include", "met2_hip.h")) as f:
        text = f.read()
    m = re.search(r"\bint\s+met2_degibbs\s*\(([^;]*)\)\s*;", text)
    assert m
    ctype = {"int32_t": C.c_int32, "const double *": C.c_void_p, "double *": C.c_void_p, "int8_t *": C.c_void_p, "void *": C.c_void_p}
    want = []
    for arg in m.group(1).split(","):
        kind = re.sub(r"\w+$", "", " ".join(arg.split())).strip()       # drop the parameter's name
        want.append(ctype[kind])
    assert len(want) == 13
    assert list(L.met2_degibbs.argtypes) == want


@pytest.mark.parametrize("n", [8, 9, 16, 65, 128])
def test_fft_and_convolution_forms_of_the_shifts_agree(n):
    x = 100.0 + 5.0 * np.random.default_rng(n).standard_normal((3, n))
    a = gn.shifted_lines_fft(x, 20)
    b = gn.shifted_lines_conv(x, 20)
    assert a.shape == (3, 41, n)
    err = np.abs(a - b).max() / np.abs(x).max()
    print("n = %d: max |fft - conv| / max|x| = %.2e" % (n, err))
    assert err <= 1e-12
    assert np.abs(a[:, 0] - x).max() <= 1e-12 * np.abs(x).max()      # shift 0 is the line itself, Nyquist bin included
    if n % 2 == 0:                                                   # every other shift drops the Nyquist bin: the shifted line holds none
        alt = (-1.0) ** np.arange(n)
        assert np.abs(a[:, 1:] @ alt).max() <= 1e-9 * np.abs(x).max()
        assert np.abs(x @ alt).min() > 1.0


def test_zero_and_constant_slices():
    z = gn.degibbs(np.zeros((12, 9, 1, 1)))
    assert not z["out"].any() and not z["shift_x"].any() and not z["shift_y"].any()
    for shape in ((12, 9, 1, 1), (8, 16, 1, 1)):
        c = gn.degibbs(np.full(shape, 37.5))
        assert np.abs(c["out"] - 37.5).max() <= 1e-12 * 37.5


def test_non_finite_slice_is_copied_through():
    data, _ = gn.case("mixed")
    bad = data.copy()
    bad[3, 4, 1, 0] = np.nan
    a, b = gn.degibbs(data), gn.degibbs(bad)
    assert np.array_equal(b["out"][:, :, 1, 0], bad[:, :, 1, 0], equal_nan=True)
    keep = np.ones(data.shape[2:], dtype=bool)
    keep[1, 0] = False
    assert np.array_equal(a["out"][:, :, keep], b["out"][:, :, keep])


def test_unringing_commutes_with_a_circular_roll():
    x = 100.0 + 5.0 * np.random.default_rng(5).standard_normal((4, 24))
    out, sh, gap = gn.unring_lines(x)
    assert gap.min() > 1e-6                                          # no tie, so the shifts must roll with the line
    for k in (1, 7, 23):
        o2, s2, _ = gn.unring_lines(np.roll(x, k, axis=-1))
        assert np.array_equal(s2, np.roll(sh, k, axis=-1))
        assert np.abs(o2 - np.roll(out, k, axis=-1)).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("shape", [(8, 8), (9, 15), (16, 12), (16, 9)])
def test_split_reproduces_the_slice_less_its_corner_nyquist_term(shape):
    nx, ny = shape
    S = 100.0 + 5.0 * np.random.default_rng(nx * ny).standard_normal(shape)
    ix, iy = gn.split2d(S)
    want = S.copy()
    if nx % 2 == 0 and ny % 2 == 0:
        sign = (-1.0) ** (np.arange(nx)[:, None] + np.arange(ny)[None, :])
        want -= (S * sign).sum() / (nx * ny) * sign
        assert np.abs(want - S).max() > 1e-6
    assert np.abs(ix + iy - want).max() <= 1e-12 * np.abs(S).max()
    gx, gy = gn.split_weights(nx, ny)
    assert np.all((gx >= 0) & (gx <= 1)) and np.all((gx + gy == 0) | (np.abs(gx + gy - 1) < 1e-15))


@pytest.mark.parametrize("name", sorted(gn.CASES))
def test_committed_volumes_hold_no_ties(name):
    data, (nsh, minW, maxW) = gn.case(name)
    res = gn.degibbs(data, nsh, minW, maxW)
    m = min(res["margin_x"].min(), res["margin_y"].min())
    print("%s: smallest margin %.2e" % (name, m))
    assert not gn.ties(res).any(), m


@pytest.mark.parametrize("name", gn.IMAGES)
def test_committed_images_hold_no_ties(name):
    data = gn.image_volume(name)
    res = gn.degibbs(data)
    m = min(res["margin_x"].min(), res["margin_y"].min())
    print("%s %s: smallest margin %.2e" % (name, data.shape, m))
    assert not gn.ties(res).any(), m
    if name == "box":
        assert (data == 0.0).sum() > data.size // 2
    if name == "scales":
        assert data.shape[3] == 3 and np.array_equal(data[:, :, 0, 2], data[:, :, 0, 1] * 1e7)


@pytest.mark.parametrize("n,params", gn.line_cases())
def test_committed_lines_hold_few_ties(n, params):
    """the line sets of tests/test_gpu_gibbs_kernels.py, in the extended-precision restatement alone: no sample of the noise lines is a tie,
    at most 2 % of the samples of the designed lines are (their all-zero line is one all along)"""
    noise = gn.line_reference(n, params, "noise")
    assert (noise["margin"] >= gn.TIE).all(), noise["margin"].min()
    des = gn.line_reference(n, params, "designed")
    share = float((des["margin"] < gn.TIE).mean())
    z = des["zero_at"]
    print("n = %d %s: noise lines' smallest margin %.2e; designed lines: %d, %.2f %% of the samples are ties (%d outside the zero line)"
          % (n, params, noise["margin"].min(), des["lines"].shape[0], 100 * share, int((np.delete(des["margin"], z, axis=0) < gn.TIE).sum())))
    assert share <= 0.02
    assert not des["shift"][z].any() and not des["out"][z].any() and not des["best"][z].any()
    assert 2 * (params[2] + 1) <= n


def test_extended_precision_routes_agree_with_the_float64_ones():
    x = gn.noise_lines(16)
    o, s, g, b = gn.ld_unring_lines(x)
    o2, s2, g2 = gn.unring_lines(x)
    assert np.array_equal(s, s2) and np.abs(o - o2).max() <= 1e-12 * np.abs(x).max()
    S = 100.0 + 5.0 * np.random.default_rng(3).standard_normal((16, 12))
    ix, iy, corner = gn.ld_split2d(S)
    a, c = gn.split2d(S)
    assert max(np.abs(ix - a).max(), np.abs(iy - c).max()) <= 1e-12 * np.abs(S).max()
    assert np.abs(gn.ld_shift_kernels(9, 20) - gn.shift_kernels(9, 20)).max() <= 1e-12


def test_known_answer_disc():
    img, dist = gn.disc_phantom()
    assert img.shape == (64, 64)
    out = gn.degibbs(img[:, :, None, None])["out"][:, :, 0, 0]
    inside = dist <= 0.3 * 64 - 3.0                                  # inside the disc, 3 pixels clear of its edge
    assert inside.sum() > 500
    s0, s1 = img[inside].std(), out[inside].std()
    p0, p1 = img.max() - 120.0, out.max() - 120.0
    print("oscillation inside the disc %.3f -> %.3f (factor %.1f), overshoot above 120: %.2f -> %.2f" % (s0, s1, s0 / s1, p0, p1))
    assert s0 > 0.5 and p0 > 5.0                                     # the phantom does ring
    assert s1 <= s0 / 4.0
    assert p1 <= p0 / 2.0
    assert abs(out[inside].mean() - 120.0) < 0.5
