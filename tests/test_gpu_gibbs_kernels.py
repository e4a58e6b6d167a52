"""The kernels of met2_degibbs (csrc/met2_gibbs.hip) stage by stage, through the diagnostic entries met2_gibbs_tables, met2_gibbs_split and
met2_gibbs_lines (gibbs.py), which launch them through the host code met2_degibbs itself runs: the tables, the 2-D split (gather, the three
DFT kernels, scatter) and the line operator U, each against the header's formulas in extended precision (tests/tools/gibbs_numpy.py, ld_*: a
dense DFT and the cosine sums, no numpy.fft).

Bounds.  1e-12 max|x| is what tests/test_gibbs_host.py holds two correct float64 formulations to; a float64 sum of n <= 256 products of
unit-size factors is good to about n 2^-53 = 3e-14, forty times below.  The winning total variation `best` is a sum of maxW - minW + 1
absolute differences of two shifted samples, each within the bound: 2 (maxW - minW + 1) 1e-12 max|line|.  The shift is discrete: it is
compared wherever the reference's own margin is at least gn.TIE; tests/test_gibbs_host.py asserts how few samples that leaves out.  Every
test prints the largest deviation it measured."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import gibbs_numpy as gn                                           # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
PREC = "long double" if gn.LD_IS_WIDER else "float64 (this platform's long double is no wider)"


@pytest.fixture(scope="module")
def gibbs():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".gibbs")


@pytest.fixture(scope="module")
def motor(gibbs):
    return importlib.import_module(PKG + ".motor")


@pytest.mark.parametrize("nsh", [1, 3, 20, 32])
@pytest.mark.parametrize("n", [8, 9, 16, 65, 128, 255, 256])
def test_tables(gibbs, n, nsh):
    W, c = gibbs.gibbs_tables(n, nsh)
    nj = 2 * nsh + 1
    jp = gibbs.gibbs_table_cols(nsh)
    assert jp >= nj and jp % 7 == 0 and jp - nj < 7
    assert W.shape == (n, n) and c.shape == (n, jp)
    wr, wi = gn.ld_dft_matrix(n)
    cref = gn.ld_shift_kernels(n, nsh)                               # [j, r]
    eW = float(max(np.abs(W.real - wr).max(), np.abs(W.imag - wi).max()))
    ec = float(np.abs(c[:, :nj] - cref.T).max())
    esum = float(np.abs(c[:, :nj].astype(gn.LD).sum(axis=0) - 1).max())
    unit = np.zeros(n)
    unit[0] = 1.0
    e0 = float(np.abs(c[:, 0] - unit).max())
    print("tables n = %d nsh = %d (%s): max |W - ref| = %.2e, |c - ref| = %.2e, |sum c_j - 1| = %.2e, |c_0 - unit| = %.2e"
          % (n, nsh, PREC, eW, ec, esum, e0))
    gn.record("tables/n%d_nsh%d" % (n, nsh), {"W": eW, "c": ec, "sum": esum, "c0": e0})
    assert eW <= 1e-12
    assert ec <= 1e-12
    assert not c[:, nj:].any()                                       # the padding is exactly 0
    assert esum <= 1e-12
    assert e0 <= 1e-12
    if n % 2 == 0:
        assert W[1, n // 2].real == -1.0 and W[n // 2, 1].real == -1.0      # the split's den == 0 rests on it


SPLIT_SHAPES = [(8, 8), (9, 15), (16, 9), (16, 12), (12, 20), (65, 64), (33, 128), (256, 256)]


@pytest.mark.parametrize("shape", SPLIT_SHAPES)
def test_split(gibbs, shape):
    nx, ny = shape
    nz, nt = (2, 1) if nx * ny > 10000 else (3, 2)                   # nx no multiple of 8: a row group of the DFT kernels straddles two slices
    rng = np.random.default_rng(nx * 1000 + ny)
    data = 100.0 + 5.0 * rng.standard_normal((nx, ny, nz, nt))
    data[:, :, 1, 0] *= 1e-4                                         # a small slice next to large ones: the error is taken per slice
    ix, iy = gibbs.gibbs_split(data)
    assert ix.shape == iy.shape == data.shape
    ex = ey = es = 0.0
    for z in range(nz):
        for e in range(nt):
            S = data[:, :, z, e]
            rx, ry, corner = gn.ld_split2d(S)
            scale = np.abs(S).max()
            if nx % 2 == 0 and ny % 2 == 0:
                assert np.abs(corner).max() > 1e-6 * scale
            else:
                assert not corner.any()
            ex = max(ex, float(np.abs(ix[:, :, z, e] - rx).max() / scale))
            ey = max(ey, float(np.abs(iy[:, :, z, e] - ry).max() / scale))
            es = max(es, float(np.abs(ix[:, :, z, e].astype(gn.LD) + iy[:, :, z, e] - (S - corner)).max() / scale))
    print("split %s x %d slices (%s): max per slice |Ix - ref| = %.2e, |Iy - ref| = %.2e, |Ix + Iy - (S - corner)| = %.2e, over max|slice|"
          % (shape, nz * nt, PREC, ex, ey, es))
    gn.record("split/%dx%d" % shape, {"Ix": ex, "Iy": ey, "sum": es})
    assert ex <= 1e-12 and ey <= 1e-12
    assert es <= 1e-12


@pytest.mark.parametrize("n,params", gn.line_cases())
def test_lines(gibbs, n, params):
    nsh, minW, maxW = params
    worst = {}
    for kind in ("noise", "designed"):
        ref = gn.line_reference(n, params, kind)
        lines = ref["lines"]
        if 256 // n > 1:
            assert lines.shape[0] % (256 // n) != 0                  # the last workgroup is partly idle
        out, shift, best = gibbs.gibbs_lines(lines, nsh, minW, maxW)
        assert out.shape == shift.shape == best.shape == lines.shape and shift.dtype == np.int8
        sure = ref["margin"] >= gn.TIE
        if kind == "noise":
            assert sure.all()
        wrong = int((shift != ref["shift"])[sure].sum())
        # where the shift may differ (a tie) so may the output: it is compared where the shift is the reference's
        same = shift == ref["shift"]
        eo = float((np.abs(out - ref["out"]) / ref["scale"])[same].max())
        eb = float((np.abs(best - ref["best"]) / ref["scale"]).max())
        worst[kind] = {"out": eo, "best": eb, "wrong_shifts": wrong, "left_out": int((~sure).sum()), "min_margin": float(ref["margin"][sure].min())}
        print("lines n = %d %s %s, %d lines (%s): %d shifts differ (%d samples left out as ties), max |out - ref| = %.2e, |best - ref| = %.2e "
              "over max|line|, smallest margin compared %.2e" % (n, params, kind, lines.shape[0], PREC, wrong, (~sure).sum(), eo, eb,
                                                                 ref["margin"][sure].min()))
        assert wrong == 0
        assert same[sure].all()
        assert eo <= 1e-12
        assert eb <= 2 * (maxW - minW + 1) * 1e-12
        z = ref["zero_at"]
        if z is not None:
            assert lines[z - 1].any() and lines[z + 1].any() and not lines[z].any()
            assert not shift[z].any()
            assert np.array_equal(out[z], np.zeros(n)) and np.array_equal(best[z], np.zeros(n))     # exactly
    gn.record("lines/n%d_%d_%d_%d" % ((n,) + params), worst)


@pytest.mark.parametrize("name", ["n8", "odd", "mixed", "wave", "long", "extreme", "params", "nsh32"])
def test_filter_equals_its_stages_bit_for_bit(gibbs, motor, name):
    """met2_degibbs (no output of the total variation) against the split and the line entry (with it) put together by hand"""
    data, (nsh, minW, maxW) = gn.case(name)
    out, sx, sy = motor.gibbs_filter(data, nsh, minW, maxW, return_shifts=True)
    ix, iy = gibbs.gibbs_split(data)
    nx, ny, nz, nt = data.shape
    cols = np.ascontiguousarray(ix.transpose(2, 3, 1, 0)).reshape(-1, nx)       # the lines along x
    rows = np.ascontiguousarray(iy.transpose(2, 3, 0, 1)).reshape(-1, ny)
    ox, shx, _ = gibbs.gibbs_lines(cols, nsh, minW, maxW)
    oy, shy, _ = gibbs.gibbs_lines(rows, nsh, minW, maxW)
    back_x = lambda a: a.reshape(nz, nt, ny, nx).transpose(3, 2, 0, 1)
    back_y = lambda a: a.reshape(nz, nt, nx, ny).transpose(2, 3, 0, 1)
    assert np.array_equal(back_x(shx), sx) and np.array_equal(back_y(shy), sy)
    assert np.array_equal(back_x(ox) + back_y(oy), out)


def test_return_codes_of_the_stage_entries(gibbs):
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    buf = torch.zeros(257 * 257 * 2, dtype=torch.float64, device="cuda")
    o = torch.full_like(buf, 7.0)
    o2 = torch.full_like(buf, 7.0)
    s8 = torch.full((4096,), 7, dtype=torch.int8, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()

    assert L.met2_gibbs_table_cols(0) == E_INVALID and L.met2_gibbs_table_cols(33) == E_UNSUPPORTED
    assert [L.met2_gibbs_table_cols(k) for k in (1, 3, 4, 20, 32)] == [7, 7, 14, 42, 70]

    def tables(n=16, nsh=20, W=o, c=o2):
        return L.met2_gibbs_tables(0, n, nsh, p(W), p(c), None)
    assert tables(n=7) == E_UNSUPPORTED and tables(n=257) == E_UNSUPPORTED and tables(n=-1) == E_UNSUPPORTED
    assert tables(nsh=0) == E_INVALID and tables(nsh=33) == E_UNSUPPORTED
    assert tables(W=None) == E_INVALID and tables(c=None) == E_INVALID

    def split(nx=16, ny=16, nz=1, nt=1, data=buf, ix=o, iy=o2):
        return L.met2_gibbs_split(0, nx, ny, nz, nt, p(data), p(ix), p(iy), None)
    assert split(nx=7) == E_UNSUPPORTED and split(nx=257) == E_UNSUPPORTED and split(ny=7) == E_UNSUPPORTED and split(ny=257) == E_UNSUPPORTED
    assert split(nx=-1) == E_INVALID and split(nt=-1) == E_INVALID
    assert split(data=None) == E_INVALID and split(ix=None) == E_INVALID and split(iy=None) == E_INVALID
    assert split(ix=buf) == E_INVALID and split(iy=buf) == E_INVALID and split(iy=o) == E_INVALID
    for shape in ((0, 16, 1, 1), (16, 0, 1, 1), (16, 16, 0, 1), (16, 16, 1, 0)):
        assert split(*shape) == 0

    def lines(n=16, nl=4, nsh=20, minW=1, maxW=3, x=buf, out=o, shift=s8, best=o2):
        return L.met2_gibbs_lines(0, n, nl, p(x), nsh, minW, maxW, p(out), p(shift), p(best), None)
    assert lines(n=7) == E_UNSUPPORTED and lines(n=257) == E_UNSUPPORTED
    assert lines(n=-1) == E_INVALID and lines(nl=-1) == E_INVALID
    assert lines(nsh=0) == E_INVALID and lines(nsh=33) == E_UNSUPPORTED
    assert lines(minW=0) == E_INVALID and lines(minW=3, maxW=2) == E_INVALID
    assert lines(maxW=8) == E_UNSUPPORTED and lines(n=8, maxW=4) == E_UNSUPPORTED
    assert lines(x=None) == E_INVALID and lines(out=None) == E_INVALID and lines(out=buf) == E_INVALID
    assert lines(n=256, nl=1 << 23) == E_UNSUPPORTED                   # 2^31 samples
    assert lines(nl=0) == 0 and lines(n=0) == 0 and lines(nl=0, nsh=0) == E_INVALID
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((o2 == 7.0).all()) and bool((s8 == 7).all())       # nothing was launched
    assert lines(shift=None, best=None) == 0                           # the two diagnostics are optional
    assert lines(maxW=7) == 0
    with pytest.raises(lib.Met2Error):
        gibbs.gibbs_tables(7)
    with pytest.raises(lib.Met2Error):
        gibbs.gibbs_table_cols(33)
    with pytest.raises(ValueError):
        gibbs.gibbs_split(np.zeros((16, 16, 4)))
    with pytest.raises(ValueError):
        gibbs.gibbs_lines(np.zeros(16))
