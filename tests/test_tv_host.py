"""CPU tests of the TV denoiser's host side.  (1) oracle/tv_oracle.py's 'ddd' coefficients against a second transcription that shares no
code with it: numpy's own half-sample symmetric extension (np.pad, mode 'symmetric') instead of the index formula `_reflect` -- which
csrc/met2_tv.hip's reflect_idx repeats -- and long double arithmetic.  (2) met2_tv_launch_info (host only) against the tile rule
include/met2_hip.h documents, at the sizes on either side of every seam, and met2_tv_work_bytes against it.  (3) the energies the
restatement of Chambolle's iteration can return."""
import importlib

import numpy as np
import pytest

from oracle import tv_oracle

PKG = "multicomponent-t2-toolbox_amd"

# every axis length 1..9 on each axis in turn (odd lengths, lengths below the four taps, a singleton axis; the other two axes at 5),
# and one volume with a length on either side of a wave on each axis
DETAIL_SHAPES = sorted({tuple(n if a == ax else 5 for a in range(3)) for ax in range(3) for n in range(1, 10)}) + [(63, 64, 65)]


def ddd_longdouble(vol):
    """pywt.dwtn(vol, 'db2', mode='symmetric')['ddd'] written from its definition: per axis the signal is extended by four samples on
    either side (more than the three a filter of four taps can reach), d[o] = sum_j g[j] x_ext[2 o + 1 - j], o < (n + 3) // 2."""
    g = np.array(tv_oracle.DB2_DEC_HI, dtype=np.longdouble)
    d = np.asarray(vol, dtype=np.longdouble)
    for ax in range(d.ndim):
        n = d.shape[ax]
        ext = np.pad(d, [(4, 4) if a == ax else (0, 0) for a in range(d.ndim)], mode="symmetric")
        o = np.arange((n + 3) // 2)
        d = sum(g[j] * np.take(ext, 2 * o + 1 - j + 4, axis=ax) for j in range(4))
    return d


def test_numpy_symmetric_padding_repeats_the_reflection_on_short_axes():
    """The premise of ddd_longdouble at n = 1, 2, 3, where the pad of four is longer than the signal: np.pad keeps reflecting
    (... c b a | a b c | c b a a b c ...), written out by hand here."""
    assert np.array_equal(np.pad([7.0], 4, mode="symmetric"), [7.0] * 9)
    assert np.array_equal(np.pad([1.0, 2.0], 4, mode="symmetric"), [1, 2, 2, 1, 1, 2, 2, 1, 1, 2])
    assert np.array_equal(np.pad([1.0, 2.0, 3.0], 4, mode="symmetric"), [3, 3, 2, 1, 1, 2, 3, 3, 2, 1, 1])
    assert np.array_equal(np.pad([1.0, 2.0, 3.0, 4.0, 5.0], 4, mode="symmetric"), [4, 3, 2, 1, 1, 2, 3, 4, 5, 5, 4, 3, 2])


def test_oracle_detail_coefficients_match_a_second_transcription():
    """Bound: three passes of four separately rounded products and three additions each, |d| <= (sum |g|)^3 max|x| = 4.68 max|x|:
    9 x 2^-53 x 4.68 = 4.7e-15 max|x|; doubled and rounded up, 1e-14 max|x| absolute."""
    rng = np.random.default_rng(17)
    for shape in DETAIL_SHAPES:
        vol = rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 3, shape)
        got = tv_oracle.detail_coefficients(vol)
        ref = ddd_longdouble(vol)
        assert got.shape == ref.shape == tuple((n + 3) // 2 for n in shape)
        err = float(np.max(np.abs(got.astype(np.longdouble) - ref)))
        assert err <= 1e-14 * np.max(np.abs(vol)), (shape, err / np.max(np.abs(vol)))
    # the transcription itself: a constant is annihilated on every axis length, borders included (the filter sums to zero to 1e-11)
    for shape in DETAIL_SHAPES[:12]:
        assert float(np.max(np.abs(ddd_longdouble(np.full(shape, 3.0))))) < 1e-10


def test_oracle_chambolle_returns_its_energies():
    rng = np.random.default_rng(2)
    img = 50.0 * (np.arange(9)[:, None, None] > 4) + rng.standard_normal((9, 7, 6))
    out, n, E = tv_oracle.denoise_tv_chambolle(img, 4.0, return_iters=True, return_energies=True)
    assert len(E) == n > 2 and all(isinstance(e, float) for e in E)
    thr = 2.0e-4 * E[0]
    assert abs(E[-2] - E[-1]) < thr and all(abs(E[i - 1] - E[i]) >= thr for i in range(1, n - 1))     # the stopping rule, read off the list
    out2, E2 = tv_oracle.denoise_tv_chambolle(img, 4.0, return_energies=True)
    assert np.array_equal(out2, out) and E2 == E
    assert np.array_equal(tv_oracle.denoise_tv_chambolle(img, 4.0), out)                                # the default is unchanged
    o3, n3 = tv_oracle.denoise_tv_chambolle(img, 4.0, max_num_iter=3, return_iters=True)
    assert n3 == 3 and tv_oracle.denoise_tv_chambolle(img, 4.0, max_num_iter=3, return_energies=True)[1] == E[:3]


# ---- met2_tv_launch_info ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tv():
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".tv")


def test_tv_launch_info_is_the_documented_geometry(tv):
    base = tv.tv_launch_info(20, 20, 20)
    oy, step2, xlen = base["oy"], base["step2"], base["xlen"]
    assert (oy, step2, xlen, base["sigma_cap"]) == (8, 64, 16, 6144)                # the shipped geometry, stated once: the GPU tests derive from it
    # rows: a tile that spans axis 1 owns all its rows; from oy + 1 on the last row is a halo
    g8, g9 = tv.tv_launch_info(5, 8, 5), tv.tv_launch_info(5, 9, 5)
    assert (g8["step1"], g8["nt1"]) == (oy, 1)
    assert (g9["step1"], g9["nt1"]) == (oy - 1, 2)
    for n1 in (1, 7, 8, 9, 14, 15, 16, 21, 22):
        g = tv.tv_launch_info(3, n1, 3)
        assert g["step1"] == (oy if n1 <= oy else oy - 1) and g["nt1"] == -(-n1 // g["step1"]), n1
    # lanes: 64 per tile along the contiguous axis, no overlap
    assert [tv.tv_launch_info(3, 3, n2)["nt2"] for n2 in (63, 64, 65, 128, 129)] == [1, 1, 2, 2, 3]
    # planes: segments of xlen (of n0 when the volume is thinner)
    assert [tv.tv_launch_info(n0, 3, 3)["nseg"] for n0 in (1, 2, 16, 17, 32, 33)] == [1, 1, 1, 2, 2, 3]
    assert [tv.tv_launch_info(n0, 3, 3)["xlen"] for n0 in (1, 2, 16, 17)] == [1, 2, 16, 16]
    for shape in [(17, 15, 65), (33, 9, 129), (2, 16, 128), (1, 1, 1), (40, 40, 40), (63, 64, 65)]:
        for em in (0, 1):
            g = tv.tv_launch_info(*shape, 3, em)
            n0, n1, n2 = shape[::-1] if em else shape                                # echo-major: the volume lies in memory as (z, y, x)
            assert (g["c0"], g["c1"], g["c2"]) == ((n0 + 3) // 2, (n1 + 3) // 2, (n2 + 3) // 2)
            assert g["nc"] == ((n0 + 3) // 2) * ((n1 + 3) // 2) * ((n2 + 3) // 2)
            assert g["nt2"] == -(-n2 // step2) and g["nseg"] == -(-n0 // min(n0, xlen))
            assert g["ntiles"] == g["nt1"] * g["nt2"] * g["nseg"]
    assert tv.tv_launch_info(40, 40, 40)["nc"] == 9261


def test_tv_work_bytes_is_consistent_with_the_launch_info(tv):
    L = importlib.import_module(PKG + "._lib")
    up = lambda b: (b + 255) // 256 * 256
    for shape, nt in [((17, 15, 65), 2), ((33, 9, 129), 5), ((1, 1, 1), 1), ((24, 20, 16), 4), ((3, 3, 5), 128)]:
        for em in (0, 1):
            g = tv.tv_launch_info(*shape, nt, em)
            vol = shape[0] * shape[1] * shape[2]
            want = up(8 * vol * nt) + 2 * up(24 * vol * nt) + up(8 * g["nc"] * nt) + up(16 * g["ntiles"] * nt) + up(56 * nt) + up(8 * nt)
            assert int(L.lib().met2_tv_work_bytes(*shape, nt, em)) == want, (shape, nt, em)
    with pytest.raises(L.Met2Error):
        tv.tv_launch_info(0, 4, 4)
    with pytest.raises(L.Met2Error):
        tv.tv_launch_info(4, 4, 4, 0)
    assert L.lib().met2_tv_launch_info(4, 4, 4, 1, 0, None) != 0


def test_new_tv_entries_have_no_cpu_fallback(tv):
    import torch
    L = importlib.import_module(PKG + "._lib")
    with pytest.raises(L.Met2Error):
        tv.tv_detail_coefficients(torch.zeros((4, 4, 4, 2), dtype=torch.float64))
    with pytest.raises(L.Met2Error):
        tv.tv_sigma_from_coefficients(torch.zeros((2, 9), dtype=torch.float64))
