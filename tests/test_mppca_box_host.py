"""CPU-only: the numpy restatement of MP-PCA with a box window and overlapping-patch averaging (tests/tools/mppca_box_numpy.py, the
reference of tests/test_gpu_mppca_box.py) against mppca_numpy.py and against known answers; the seeds the GPU parity tests commit to (the
restatement itself calls no voxel of them a tie); the window check of filters.py and the drivers' options; met2_mppca_box_work_bytes, which needs no device; and the two
prototypes of include/met2_hip.h against their ctypes declarations."""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import mppca_box_numpy as bx                                       # noqa: E402
import mppca_numpy as mp                                           # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"
E_INVALID, E_UNSUPPORTED = -1, -2
CAP = 1 << 30                                                      # the cap of the default work space the header states


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + "._lib").lib()


def test_cubic_window_without_averaging_is_mppca_numpy():
    for name in ("M7", "tiny", "wide"):
        data, mask, w = mp.case(name)
        ref = mp.mppca(data, mask, w)
        got = bx.mppca_box(data, mask, (w, w, w), average=False)
        for k in ("out", "sigma", "rank", "n"):
            assert np.array_equal(ref[k], got[k]), (name, k)
        assert np.array_equal(mp.ties(ref), got["tie"]) and not got["wsum"].any()


def test_averaging_returns_noiseless_rank_two_data():
    # two exponentials with smooth weights: the curves of a patch span two directions, which hold every curve of the patch, v's own among
    # them, so every vote is x_v itself (a patch that keeps more than two components, rounding dust taken for signal, holds it no less).
    # 12 echoes, 5 x 5 x 3 patches: N >= 18 >= M at the corners.
    rng = np.random.default_rng(3)
    shape, M = (6, 6, 4), 12
    te = np.arange(1, M + 1)
    basis = np.stack([np.exp(-te / 3.0), np.exp(-te / 9.0)])
    data = (1.0 + rng.random(shape + (2,))) @ basis
    mask = np.ones(shape, dtype=np.uint8)
    res = bx.mppca_box(data, mask, (5, 5, 3), average=True)
    assert res["n"].min() >= M and (res["rank"] >= 2).all() and (res["wsum"] > 0).all()
    print("ranks", np.unique(res["rank"]), "max |out - data| / max|data| = %.3e" % (np.abs(res["out"] - data).max() / np.abs(data).max()))
    assert np.abs(res["out"] - data).max() <= 1e-9 * np.abs(data).max()


def test_averaging_lowers_the_error_on_the_phantom():
    # the table of the README (CPU figures of this restatement): RMSE over the mask against the noiseless phantom
    synth = importlib.import_module(PKG + ".synth")
    noisy, mask = (t.numpy() for t in synth.make_phantom((14, 14, 6), nte=32, seed=5, snr=50, device="cpu"))
    clean = synth.make_phantom((14, 14, 6), nte=32, seed=5, snr=1e12, device="cpu")[0].numpy()
    on = mask != 0
    rmse = lambda a: float(np.sqrt(np.mean((a[on] - clean[on]) ** 2)))
    assert abs(rmse(noisy) - 14.39) < 0.005
    for window, centre, average in (((5, 5, 5), 5.38, 5.00), ((5, 5, 1), 5.93, 5.39), ((7, 7, 3), 5.17, 4.95)):
        a = rmse(bx.mppca_box(noisy, mask, window, average=False)["out"])
        b = rmse(bx.mppca_box(noisy, mask, window, average=True)["out"])
        print(window, "centre only %.4f, overlap average %.4f" % (a, b))
        assert abs(a - centre) < 0.005 and abs(b - average) < 0.005 and b < a


@pytest.mark.parametrize("name", sorted(bx.CASES))
def test_committed_cases_have_no_ties_and_meet_every_class(name):
    data, mask, window = bx.case(name)
    res = bx.mppca_box(data, mask, window, average=True)
    assert not res["tie"].any()
    assert (mask == 0).any() and not res["out"][mask == 0].any() and not res["wsum"][mask == 0].any()
    if np.prod(mask.shape) > 200:                                  # the isolated voxel: copied, rank 1, no vote
        v = (mask.shape[0] - 1, mask.shape[1] - 1, 0)
        assert res["n"][v] == 1 and res["rank"][v] == 1 and res["wsum"][v] == 0 and np.array_equal(res["out"][v], data[v])
    assert (res["wsum"][res["n"] >= 2] > 0).all()


def test_the_filter_validates_its_window():
    importlib.import_module(PKG + "._build").build()
    filters = importlib.import_module(PKG + ".filters")
    assert filters.mppca_window(5) == (5, 5, 5) and filters.mppca_window((5, 5, 1)) == (5, 5, 1)
    assert filters.mppca_window(np.array([7, 7, 3]), True) == (7, 7, 3) and filters.mppca_window(7, True) == (7, 7, 7)
    assert filters.mppca_window(9) == (9, 9, 9)                    # the cube of met2_mppca: the library decides whether it fits
    for bad in (4, 1, 0, -3, (5, 5), (5, 4, 1), (1, 1, 1), (0, 3, 3), (9, 9, 5), 2.5, (5.0, 5.0, 1.0), "5", None, (3, 3, 3, 3)):
        with pytest.raises(ValueError, match="window"):
            filters.mppca_window(bad)
    with pytest.raises(ValueError, match="343"):
        filters.mppca_window(9, True)
    assert importlib.import_module(PKG + ".motor").mppca_filter is filters.mppca_filter


def resolve(motor, method="MPPCA", denoise=dict, **mppca):                     # denoise as given, else the dict of method and **mppca
    args = dict(FA_method="brute-force", FA_smooth="no", device=0, devices=None, bootstrap=None, degibbs="no", bias_correct="no",
                voxel_size=None, brain_mask="no", segment="no", tissue_stats="no", pve_threshold=0.9, rician="no", rician_sigma=None,
                rician_iters=3, slice_profile=None)
    return motor._resolve_run((8, 8, 4, 32), np.ones((8, 8, 4)), denoise=dict(method=method, **mppca) if denoise is dict else denoise, **args)


def test_driver_options_are_validated_once():
    # the drivers' argument lists are fixed (tests/test_pve_host.py), so mppca_window and mppca_average ride in a dict-valued denoise
    importlib.import_module(PKG + "._build").build()
    motor = importlib.import_module(PKG + ".motor")
    for plain in ("MPPCA", "None", None, "TV", "NESMA"):
        run = resolve(motor, denoise=plain)
        assert run.mppca == (5, False) and run.denoise == plain
    assert resolve(motor).mppca == (5, False) and resolve(motor).denoise == "MPPCA"
    assert resolve(motor, method="TV").denoise == "TV" and resolve(motor, method="None", mppca_window=5, mppca_average="no").mppca == (5, False)
    assert resolve(motor, mppca_window=(5, 5, 1), mppca_average="yes").mppca == ((5, 5, 1), True)
    assert resolve(motor, mppca_window=np.array([7, 7, 3])).mppca == ((7, 7, 3), False)
    assert resolve(motor, mppca_window=7, mppca_average="yes").mppca == (7, True)
    assert resolve(motor, mppca_window=9).mppca == (9, False)      # the cube of met2_mppca: the library decides whether it fits
    for bad in (4, 1, 0, -3, (5, 5), (5, 4, 1), (1, 1, 1), (0, 3, 3), (9, 9, 5), 2.5, (5.0, 5.0, 1.0), "5", None, (3, 3, 3, 3)):
        with pytest.raises(ValueError, match="window"):
            resolve(motor, mppca_window=bad)
    with pytest.raises(ValueError, match="343"):
        resolve(motor, mppca_window=9, mppca_average="yes")
    for bad in ("maybe", True, 1, None):
        with pytest.raises(ValueError, match="mppca_average"):
            resolve(motor, mppca_average=bad)
    for kw in (dict(mppca_window=(5, 5, 1)), dict(mppca_window=3), dict(mppca_average="yes")):
        for method in ("None", "TV", "NESMA"):
            with pytest.raises(ValueError, match="need the denoise method 'MPPCA'"):
                resolve(motor, method=method, **kw)
    for bad in ({}, {"mppca_window": 5}, {"method": "MPPCA", "window": 5}, {"method": "PCA"}, {"method": ("MPPCA",)}, ("MPPCA", 5), 5):
        with pytest.raises(ValueError, match="denoise"):
            resolve(motor, denoise=bad)
    # rician='direct' takes the map of either mode: the dict form counts as denoise='MPPCA'
    args = dict(FA_method="brute-force", FA_smooth="no", device=0, devices=None, bootstrap=None, degibbs="no", bias_correct="no", voxel_size=None,
                brain_mask="no", segment="no", tissue_stats="no", pve_threshold=0.9, rician="direct", rician_sigma=None, rician_iters=3, slice_profile=None)
    run = motor._resolve_run((8, 8, 4, 32), np.ones((8, 8, 4)), denoise={"method": "MPPCA", "mppca_average": "yes"}, **args)
    assert run.rician == "direct" and run.mppca == (5, True)
    # both drivers hand the options to _resolve_run before any device work
    TE = 10.0 * np.arange(1, 33)
    with pytest.raises(ValueError, match="window"):
        motor.recon_met2_arrays(np.zeros((4, 4, 2, 32)), np.ones((4, 4, 2)), TE, 3000.0, denoise={"method": "MPPCA", "mppca_window": (4, 4, 1)})
    with pytest.raises(ValueError, match="need the denoise method 'MPPCA'"):
        motor.recon_met2_arrays(np.zeros((4, 4, 2, 32)), np.ones((4, 4, 2)), TE, 3000.0, denoise={"method": "None", "mppca_average": "yes"})


def work_bytes(L, shape, window, average):
    lo, dflt = C.c_int64(-1), C.c_int64(-1)
    rc = L.met2_mppca_box_work_bytes(*shape, None if window is None else (C.c_int32 * 3)(*window), average, C.byref(lo), C.byref(dflt))
    return rc, lo.value, dflt.value


def test_work_bytes_need_no_device(L):
    # the header: c centres need at most 16 + c (24 + 8 n_te K) bytes, K = min(n_te, P), P the largest patch; min_bytes is that of P centres
    most = lambda c, nt, P: 16 + c * (24 + 8 * nt * min(nt, P))
    assert work_bytes(L, (9, 8, 7, 32), (5, 5, 1), 1) == (0, most(25, 32, 25), most(504, 32, 25))
    assert work_bytes(L, (2, 8, 7, 12), (5, 5, 1), 1) == (0, most(10, 12, 10), most(112, 12, 10))          # nx = 2 clips the window
    assert work_bytes(L, (9, 8, 7, 63), (7, 7, 7), 1) == (0, most(343, 63, 343), most(504, 63, 343))
    assert most(343, 63, 343) < 11e6
    for shape, window in (((128, 128, 64, 32), (5, 5, 5)), ((128, 128, 64, 32), (5, 5, 1)), ((512, 512, 200, 63), (7, 7, 7)),
                          ((4096, 4096, 4, 63), (7, 7, 7)), ((9, 8, 7, 3), (3, 3, 1))):
        rc, lo, dflt = work_bytes(L, shape, window, 1)
        assert rc == 0 and 0 < lo <= dflt <= CAP, (shape, window, lo, dflt)
    assert work_bytes(L, (128, 128, 64, 32), (5, 5, 5), 1)[2] == CAP                # the volume's need (8.6 GB) is capped
    assert work_bytes(L, (9, 8, 7, 32), (5, 5, 1), 0) == (0, 0, 0)                  # no averaging: nothing is held
    assert work_bytes(L, (0, 8, 7, 32), (5, 5, 1), 1) == (0, 0, 0)
    for window in ((4, 5, 5), (5, 5, 0), (5, -1, 5), (1, 1, 1), None):
        assert work_bytes(L, (9, 8, 7, 32), window, 1)[0] == E_INVALID, window
    assert work_bytes(L, (9, 8, 7, 32), (5, 5, 1), 2)[0] == E_INVALID
    assert work_bytes(L, (9, 8, -7, 32), (5, 5, 1), 1)[0] == E_INVALID
    assert work_bytes(L, (9, 8, 7, 32), (7, 7, 9), 1)[0] == E_UNSUPPORTED            # 441 voxels
    assert work_bytes(L, (9, 8, 7, 64), (5, 5, 1), 1)[0] == E_UNSUPPORTED
    assert work_bytes(L, (9, 8, 7, 1), (5, 5, 1), 1)[0] == E_UNSUPPORTED
    assert L.met2_mppca_box_work_bytes(9, 8, 7, 32, (C.c_int32 * 3)(5, 5, 1), 1, None, None) == 0
    filters = importlib.import_module(PKG + ".filters")
    assert filters.mppca_work_bytes((9, 8, 7, 32), (5, 5, 1)) == (most(25, 32, 25), most(504, 32, 25))
    assert filters.mppca_work_bytes((9, 8, 7, 32), 5, average=False) == (0, 0)


def test_the_entry_checks_its_arguments_before_any_device_work(L):
    # every refusal below comes before the device is made current, so none needs one
    w = (C.c_int32 * 3)(5, 5, 1)
    call = lambda window=w, average=1, nt=32, work=0, data=8, out=16, shape=(9, 8, 7): L.met2_mppca_box(
        0, *shape, nt, data, None, window, average, work, out, None, None, None, None, None)
    assert call(window=(C.c_int32 * 3)(5, 2, 1)) == E_INVALID
    assert call(window=(C.c_int32 * 3)(1, 1, 1)) == E_INVALID
    assert call(average=-1) == E_INVALID
    assert call(nt=64) == E_UNSUPPORTED
    assert call(window=(C.c_int32 * 3)(9, 9, 5)) == E_UNSUPPORTED
    assert call(data=None) == E_INVALID and call(out=None) == E_INVALID and call(out=8) == E_INVALID
    assert call(work=-1) == E_INVALID
    lo = 16 + 25 * (24 + 8 * 32 * 25)
    assert call(work=lo - 1) == E_INVALID
    assert str(lo).encode() in L.met2_last_error()                  # the message names the minimum
    assert call(shape=(1 << 10, 1 << 10, 1 << 6)) == E_UNSUPPORTED  # 2^26 voxels
    assert call(shape=(0, 8, 7), data=None, out=None) == 0          # an empty volume: nothing to do


def test_prototypes_match_the_ctypes_declarations(L):
    lib = importlib.import_module(PKG + "._lib")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "met2_hip.h")).read(), flags=re.S)
    kinds = {"met2_mppca_box": [C.c_int32] * 5 + ["ptr", "ptr", C.POINTER(C.c_int32), C.c_int32, C.c_int64] + ["ptr"] * 6,
             "met2_mppca_box_work_bytes": [C.c_int32] * 4 + [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]}
    for name, want in kinds.items():
        assert name in lib.SYMBOLS and hasattr(L, name)
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S)
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        got = list(getattr(L, name).argtypes)
        assert len(params) == len(got) == len(want), name
        for p, t, k in zip(params, got, want):
            if k == "ptr":
                assert "*" in p and t is C.c_void_p, (name, p, t)
            elif hasattr(k, "contents"):
                base = {C.c_int32: "int32_t", C.c_int64: "int64_t"}[k._type_]
                assert base in p and ("*" in p or "[3]" in p) and t is k, (name, p, t)
            else:
                assert p.startswith({C.c_int32: "int32_t", C.c_int64: "int64_t"}[k]) and "*" not in p and t is k, (name, p, t)
    assert L.met2_abi_version() == 6
