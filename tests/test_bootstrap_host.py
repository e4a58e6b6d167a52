"""CPU-only tests of the bootstrap mode (met2_fit_bootstrap): a numpy restatement of the counter-based generator's Philox4x32-10
against Random123's known-answer vectors (the GPU tests compare the device's replicates with this restatement), and the argument
checks of the C entries and of Met2Plan.fit_bootstrap, which run before anything touches a device."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

PKG = "multicomponent-t2-toolbox_amd"

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from philox_numpy import philox4x32_10                             # noqa: E402  (moved there; shared with the Monte-Carlo study's tests)


def replicates_np(center, sigma, vid, n_rep, seed):
    """Definition 3 of met2_fit_bootstrap (include/met2_hip.h) in numpy: center [nv, n_te], sigma [nv], vid [nv] int64 -> [nv, n_rep, n_te]."""
    center = np.asarray(center, dtype=np.float64)
    nv, nte = center.shape
    vid = np.asarray(vid, dtype=np.int64).view(np.uint64)
    s = np.array([seed], dtype=np.int64).view(np.uint64)[0]
    key = (np.uint32(s & np.uint64(0xFFFFFFFF)), np.uint32(s >> np.uint64(32)))
    e = np.arange(nte, dtype=np.uint32)[None, None, :]
    b = np.arange(n_rep, dtype=np.uint32)[None, :, None]
    lo = (vid & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None, None]
    hi = (vid >> np.uint64(32)).astype(np.uint32)[:, None, None]
    shape = (nv, n_rep, nte)
    x0, x1, x2, x3 = philox4x32_10([np.broadcast_to(e, shape), np.broadcast_to(b, shape), np.broadcast_to(lo, shape), np.broadcast_to(hi, shape)], key)
    u1 = ((x0 >> 5).astype(np.float64) * 2.0 ** 26 + (x1 >> 6).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = ((x2 >> 5).astype(np.float64) * 2.0 ** 26 + (x3 >> 6).astype(np.float64)) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    z1, z2 = r * np.cos((2.0 * np.pi) * u2), r * np.sin((2.0 * np.pi) * u2)
    sg = np.asarray(sigma, dtype=np.float64)[:, None, None]
    return np.sqrt((center[:, None, :] + sg * z1) ** 2 + (sg * z2) ** 2)


def _words(*xs):
    return ["%08x" % int(x) for x in xs]


def test_philox_known_answers():
    # Random123's kat_vectors for philox4x32_10
    assert _words(*philox4x32_10([0, 0, 0, 0], [0, 0])) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert _words(*philox4x32_10([f, f, f, f], [f, f])) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _words(*philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_replicates_np_uniforms_and_zero_sigma():
    # u1 in (0, 1] keeps log finite; sigma = 0 gives the centre back exactly
    c = np.abs(np.random.default_rng(1).normal(size=(5, 8))) * 100.0
    r = replicates_np(c, np.zeros(5), np.arange(5) + 2 ** 40, 7, -1)
    assert np.array_equal(r, np.broadcast_to(c[:, None, :], r.shape))
    r = replicates_np(c, np.full(5, 3.0), np.arange(5), 7, 0)
    assert np.all(np.isfinite(r)) and np.all(r >= 0.0)
    assert not np.array_equal(r[:, 0], r[:, 1])


def _lib():
    b = importlib.import_module(PKG + "._build")
    b.build()
    lib = importlib.import_module(PKG + "._lib")
    return lib.lib()


def _boot(L, plan=None, n_rep=16, nvox=4, vs=32, es=1, seed=0):
    nul = C.c_void_p(0)
    return L.met2_fit_bootstrap(plan, 2, nvox, nul, vs, es, nul, nul, nul, nul, n_rep, seed, *([nul] * 10))


@pytest.mark.parametrize("kw,msg", [({"n_rep": 1}, "n_rep"), ({"n_rep": 1025}, "n_rep"), ({}, "NULL plan"), ({"nvox": -1}, "nvox"),
                                    ({"vs": 0}, "stride"), ({"es": -32}, "stride")])
def test_fit_bootstrap_argument_checks_need_no_gpu(kw, msg):
    L = _lib()
    assert _boot(L, **kw) == -1           # MET2_E_INVALID
    assert msg in L.met2_last_error().decode()


def test_bootstrap_replicates_argument_checks_need_no_gpu():
    L = _lib()
    nul = C.c_void_p(0)
    for n_rep, nvox, msg in ((1, 4, "n_rep"), (1025, 4, "n_rep"), (8, -1, "nvox"), (8, 4, "NULL plan")):
        assert L.met2_bootstrap_replicates(nul, nvox, nul, nul, nul, n_rep, 0, nul, nul) == -1
        assert msg in L.met2_last_error().decode()


def _series(L, n_rep=16, nvox=4, n_quant=7, values=1, stats=1):
    # nonzero "pointers" are never dereferenced: every check below fails before a device is touched
    return L.met2_bootstrap_series_stats(0, nvox, n_rep, n_quant, C.c_void_p(values * 256), C.c_void_p(0), C.c_void_p(stats * 256), C.c_void_p(0))


def _spectrum(L, n_rep=16, nvox=4, nt2=60, fsol=1, spec=1):
    return L.met2_bootstrap_spectrum_stats(0, nvox, n_rep, nt2, C.c_void_p(fsol * 256), C.c_void_p(0), C.c_void_p(spec * 256), C.c_void_p(0))


@pytest.mark.parametrize("fn,kw,msg", [(_series, {"n_rep": 1}, "n_rep"), (_series, {"n_rep": 1025}, "n_rep"), (_series, {"n_quant": 0}, "n_quant"),
                                       (_series, {"n_quant": 9}, "n_quant"), (_series, {"nvox": -1}, "nvox"), (_series, {"values": 0}, "NULL"),
                                       (_series, {"stats": 0}, "NULL"), (_spectrum, {"n_rep": 1}, "n_rep"), (_spectrum, {"n_rep": 1025}, "n_rep"),
                                       (_spectrum, {"nt2": 0}, "n_t2"), (_spectrum, {"nvox": -1}, "nvox"), (_spectrum, {"fsol": 0}, "NULL"),
                                       (_spectrum, {"spec": 0}, "NULL")])
def test_stats_entries_argument_checks_need_no_gpu(fn, kw, msg):
    L = _lib()
    assert fn(L, **kw) == -1              # MET2_E_INVALID
    assert msg in L.met2_last_error().decode()


def test_stats_entries_take_an_empty_call():
    L = _lib()
    assert _series(L, nvox=0, values=0, stats=0) == 0 and _spectrum(L, nvox=0, fsol=0, spec=0) == 0


def _next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def test_spec_launch_info_is_the_documented_geometry():
    """met2_bootstrap_spec_launch_info (host only) against the rule the kernel's comment states: 64 bins per tile up to 64 sort slots, then
    4096 / P down to 4; one double of padding from 16 bins up, 16 / w below; LDS = the [w][S] tile and the [5][w] results, under 64 KiB."""
    L = _lib()
    w, S, lds = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    for bad in (1, 1025):
        assert L.met2_bootstrap_spec_launch_info(bad, C.byref(w), C.byref(S), C.byref(lds)) == -1
    seen = set()
    for n_rep in range(2, 1025):
        assert L.met2_bootstrap_spec_launch_info(n_rep, C.byref(w), C.byref(S), C.byref(lds)) == 0
        P = _next_pow2(n_rep)
        ww = 64 if P <= 64 else 4096 // P
        assert w.value == ww and S.value == P + (1 if ww >= 16 else 16 // ww), n_rep
        assert lds.value == 8 * (ww * S.value + 5 * ww) and lds.value <= 65536, n_rep
        seen.add(ww)
    assert seen == {64, 32, 16, 8, 4}
    assert L.met2_bootstrap_spec_launch_info(64, None, None, None) == 0


def test_stats_wrappers_reject_malformed_calls_before_the_device():
    plan_mod = importlib.import_module(PKG + ".plan")
    P = plan_mod.Met2Plan
    with pytest.raises(ValueError, match="CUDA"):
        P.bootstrap_series_stats(torch.zeros((3, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_rep"):
        P.bootstrap_series_stats(torch.zeros((3, 1), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_quant"):
        P.bootstrap_series_stats(torch.zeros((9, 3, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="tensor"):
        P.bootstrap_series_stats(np.zeros((3, 8)))
    with pytest.raises(ValueError, match="CUDA"):
        P.bootstrap_spectrum_stats(torch.zeros((3, 8, 60), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_rep"):
        P.bootstrap_spectrum_stats(torch.zeros((3, 1025, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_t2"):
        P.bootstrap_spectrum_stats(torch.zeros((3, 8, 0), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_rep, n_t2"):
        P.bootstrap_spectrum_stats(torch.zeros((3, 8), dtype=torch.float64))
    assert P.bootstrap_spec_launch_info(1024) == (4, 1028, 8 * (4 * 1028 + 20))


def test_any_64bit_seed_passes_the_checks():
    L = _lib()
    for seed in (0, -1, 2 ** 63 - 1, -2 ** 63):
        assert _boot(L, seed=seed) == -1 and "NULL plan" in L.met2_last_error().decode()


def test_fit_bootstrap_rejects_malformed_calls_before_the_device():
    plan_mod = importlib.import_module(PKG + ".plan")
    p = plan_mod.Met2Plan.__new__(plan_mod.Met2Plan)          # shape only: every check below fails before the handle or a device is used
    p.n_te, p.n_t2, p.n_fa, p._h, p.device = 32, 60, 1, C.c_void_p(0), torch.device("cuda", 0)
    d = torch.zeros((4, 32), dtype=torch.float64)
    with pytest.raises(ValueError, match="unknown reg_method"):
        p.fit_bootstrap("X3", d)
    with pytest.raises(ValueError, match="float64"):
        p.fit_bootstrap("X2", d.to(torch.float32))
    with pytest.raises(ValueError, match="n_te"):
        p.fit_bootstrap("X2", torch.zeros((4, 31), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_te"):
        p.fit_bootstrap("X2", torch.zeros((32,), dtype=torch.float64))
    with pytest.raises(ValueError, match="n_rep"):
        p.fit_bootstrap("X2", d, n_rep=1)
    with pytest.raises(ValueError, match="n_rep"):
        p.fit_bootstrap("X2", d, n_rep=1025)
    with pytest.raises(ValueError, match="sigma"):
        p.fit_bootstrap("X2", d, sigma=np.array([1.0, -1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="sigma"):
        p.fit_bootstrap("X2", d, sigma=np.ones(3))
    with pytest.raises(ValueError, match="voxel_id"):
        p.fit_bootstrap("X2", d, voxel_id=np.arange(5))


def test_boot_names_exported():
    pkg = importlib.import_module(PKG)
    assert pkg.BOOT_QUANTITIES == pkg.MAP_NAMES + ("reg",)
    assert len(pkg.BOOT_STATS) == 5 and pkg.BOOT_STATS[:2] == ("mean", "std")
