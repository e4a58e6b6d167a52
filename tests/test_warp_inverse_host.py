"""The inverse of a displacement field and its Jacobian determinant without a device: the rules of met2_warp_invert_step and
met2_warp_jacobian (include/met2_hip.h) as tests/tools/warp_inverse_numpy.py restates them, and the loop of warp.invert run with that
restatement as its step.
Closed form.  u(x) = M x + t with A the identity on 20 x 18 x 16 has the inverse v(y) = (I + M)^-1 (y - t) - y wherever the pre-image lies in the
grid; u is linear, so trilinear interpolation is exact and 40 steps reach it to rounding (measured 4.2e-15 over 77 % of the voxels; bound
1e-12), the residual falling by |M|'s contraction factor per step (measured 0.10 .. 0.11).
Smooth field.  u of 1.5 voxels amplitude (smooth_field) with A = R diag(1.1, 0.9, 1.0), R 0.1 rad about z, onto 22 x 17 x 16: the residual is
below 1e-5 voxel by step 20 and below 1e-8 by step 30 (measured 2.1e-6 and 2.5e-9, ratio about 0.5).  The invariant: at every destination
voxel whose unclamped c is inside, |A (c + u_tri(c)) - y| <= 2 |L|_inf (last residual) -- with e = v_30 - v_29 the left side is L (-e) up to
the next step's change, itself below the last residual (measured 1.1e-9 at a residual of 2.5e-9, over 76 % of the voxels).
Rounding.  fp64 and long double agree to 1e-13 on every case: the iteration does not amplify rounding, which is what lets the device be held
to long double after 25 steps (tests/test_gpu_warp_inverse.py)."""
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import warp_numpy as wn                                            # noqa: E402
import warp_inverse_numpy as wi                                    # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"
LD = np.longdouble


@pytest.fixture(scope="module")
def warp():
    return importlib.import_module(PKG + ".warp")


@pytest.fixture(scope="module")
def linear():
    u = wi.linear_field()
    return u, {dt: wi.invert(u, wi.IDENTITY, wi.GRID, 40, dt) for dt in (np.float64, LD)}


@pytest.fixture(scope="module")
def smooth():
    u, A = wi.smooth_field(), wi.smooth_transform()
    return u, A, {dt: wi.invert(u, A, wi.SMOOTH_DST, 30, dt) for dt in (np.float64, LD)}


# ---------------------------------------------------------------- the closed form

def test_linear_field_reaches_the_closed_form(linear):
    u, inv = linear
    want, ok = wi.linear_inverse()
    assert 0.7 < ok.mean() < 0.85
    for dt in (np.float64, LD):
        err = np.abs(inv[dt]["disp"] - want)[ok].max()
        print("%s: |v - closed form| = %.3g over %.1f %% of the voxels" % (np.dtype(dt).name, err, 100 * ok.mean()))
        assert err <= 1e-12
    res = inv[LD]["residual"]
    ratio = res[1:12] / res[:11]
    print("residual ratios", ratio)
    assert np.all((ratio > 0.09) & (ratio < 0.12))


def test_constant_field_is_done_after_one_step():
    u = np.broadcast_to(wi.LINEAR_T, wi.GRID + (3,)).copy()
    B, N = wi.inverse_matrices(wi.IDENTITY)
    for dt in (np.float64, LD):
        v1, r1 = wi.invert_step(u, B, N, wi.GRID, None, return_res2=True, dtype=dt)
        assert np.array_equal(np.asarray(v1, dtype=np.float64), np.broadcast_to(-wi.LINEAR_T, wi.GRID + (3,)))
        assert float(r1) == float((0.5 * 0.5 + 0.25 * 0.25) + 0.125 * 0.125)
        # the second step changes nothing: a constant is interpolated exactly (the weights of a tap pair add up to 1 exactly in binary
        # fractions of 1/8) -- at every voxel, clamped or not, so wherever no coordinate is clamped in particular
        v2, ins, r2, c = wi.invert_step(u, B, N, wi.GRID, np.asarray(v1, dtype=np.float64), True, True, dt, True)
        d = np.asarray(v2, dtype=np.float64) - np.asarray(v1, dtype=np.float64)
        assert 0 < ins.sum() < ins.size and not d[ins != 0].any() and float(r2) == 0.0


# ---------------------------------------------------------------- the smooth field

def test_smooth_field_residual_and_invariant(smooth):
    u, A, inv = smooth
    norm_L = np.abs(A[:, :3]).sum(axis=1).max()
    for dt in (np.float64, LD):
        res = inv[dt]["residual"]
        print("%s: residual after 20, 25, 30 steps: %.3g %.3g %.3g" % (np.dtype(dt).name, res[19], res[24], res[29]))
        assert res.shape == (30,) and res[19] < 1e-5 and res[29] < 1e-8
        assert np.all(res[10:] / res[9:-1] < 0.7)
        err, ins = wi.round_trip_error(u, A, inv[dt], dt)
        print("invariant: %.3g <= %.3g over %.1f %% of the voxels" % (float(err[ins].max()), 2 * norm_L * res[-1], 100 * ins.mean()))
        assert 0.7 < ins.mean() < 0.85
        assert float(err[ins].max()) <= 2.0 * norm_L * res[-1]


def test_no_coordinate_of_the_smooth_case_is_near_a_face(smooth):
    # tests/test_gpu_warp_inverse.py leaves voxels out of the `inside` comparison whose c lies within 1e-9 of a face: here there is none,
    # after 25 steps (what the device test runs) as after 30
    u, A, inv = smooth
    for c in (inv[LD]["coords"], wi.invert(u, A, wi.SMOOTH_DST, 25, LD)["coords"]):
        for a in range(3):
            assert min(np.abs(c[a]).min(), np.abs(c[a] - (wi.GRID[a] - 1)).min()) > 1e-9


# ---------------------------------------------------------------- the Jacobian determinant

def test_jacobian_of_a_linear_field_is_exact_at_every_voxel():
    want = np.linalg.det(np.eye(3) + wi.LINEAR_M)
    for dt in (np.float64, LD):
        det, n = wi.jacobian(wi.linear_field(), 1.0, dt)
        err = float(np.abs(det - want).max())
        print("%s: |det - det(I + M)| = %.3g" % (np.dtype(dt).name, err))
        assert det.shape == wi.GRID and err <= 1e-14 and n == 0


@pytest.mark.parametrize("grid", wi.JACOBIAN_GRIDS)
def test_jacobian_zero_and_folded_fields(grid):
    for dt in (np.float64, LD):
        det, n = wi.jacobian(np.zeros(tuple(grid) + (3,)), 0.7, dt)
        assert np.array_equal(np.asarray(det, dtype=np.float64), np.full(grid, 0.7)) and n == 0
        det, n = wi.jacobian(np.zeros(tuple(grid) + (3,)), -1.0, dt)
        assert n == int(np.prod(grid))
        det, n = wi.jacobian(wi.folded_field(grid), 1.0, dt)
        if grid[0] > 1:
            assert np.array_equal(np.asarray(det, dtype=np.float64), np.full(grid, -0.5)) and n == int(np.prod(grid))
        else:
            assert np.array_equal(np.asarray(det, dtype=np.float64), np.ones(grid)) and n == 0      # an axis of length 1: D = 0
    u = wn.case_field(grid)
    u[0, 0, 0, 1] = np.nan
    det, n = wi.jacobian(u)
    if max(grid) > 1:
        assert n >= 1 and np.isnan(det[0, 0, 0])                   # a determinant that is not a number counts
    else:
        assert n == 0 and det[0, 0, 0] == 1.0                      # every difference is 0 by the rule: the field is not read


def test_designed_folds_sit_on_either_side_of_a_block_seam():
    u, folds = wi.designed_folds()
    det, n = wi.jacobian(u)
    assert np.array_equal(np.flatnonzero(~(det.reshape(-1) > 0)), folds) and n == folds.size
    assert {255, 256, 511, 512, det.size - 1} <= set(folds.tolist())


# ---------------------------------------------------------------- rounding

def test_fp64_and_long_double_agree(linear, smooth):
    _, lin = linear
    u, A, sm = smooth
    pairs = [(lin[np.float64]["disp"], lin[LD]["disp"]), (lin[np.float64]["residual"], lin[LD]["residual"]),
             (sm[np.float64]["disp"], sm[LD]["disp"]), (sm[np.float64]["residual"], sm[LD]["residual"])]
    for field in (wi.linear_field(), wi.smooth_field(), wi.folded_field(wi.GRID)):
        pairs.append((np.asarray(wi.jacobian(field, 1.0, np.float64)[0], dtype=np.float64), wi.jacobian(field, 1.0, LD)[0]))
    const = np.broadcast_to(wi.LINEAR_T, wi.GRID + (3,)).copy()
    B, N = wi.inverse_matrices(wi.IDENTITY)
    pairs.append((wi.invert_step(const, B, N, wi.GRID, dtype=np.float64), wi.invert_step(const, B, N, wi.GRID, dtype=LD)))
    for got, want in pairs:
        err = float(np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).max())
        assert err <= 1e-13, err
    assert np.array_equal(sm[np.float64]["inside"], sm[LD]["inside"]) and np.array_equal(lin[np.float64]["inside"], lin[LD]["inside"])


# ---------------------------------------------------------------- the label round trip the device test is held to

def test_recorded_label_recovery_is_the_restatements():
    import json
    rec = json.load(open(os.path.join(ROOT, "profiles", "warp_inverse_recovery.json")))
    lab, la, fa, A, u, truth = wi.round_trip_inputs()
    inv = wi.invert(u, A, lab.shape, rec["n_iter"], np.float64)
    share, n = wi.label_share(wn.warp_labels(truth, inv["B"], inv["disp"]), lab)
    print("labels recovered: %.4f of %d; last residual %.3g" % (share, n, inv["residual"][-1]))
    assert n == rec["n_labelled"] and abs(share - rec["share_recovered"]) < 1e-12 and share > 0.95 and rec["margin_share"] == 0.005
    assert wi.jacobian(u, 1.0, np.float64)[1] == rec["n_nonpositive"] == 0


# ---------------------------------------------------------------- the host side of the library

def test_symbols_and_abi():
    lib = importlib.import_module(PKG + "._lib")
    assert {"met2_warp_invert_step", "met2_warp_jacobian"} <= set(lib.SYMBOLS)
    L = lib.lib()
    assert hasattr(L, "met2_warp_invert_step") and hasattr(L, "met2_warp_jacobian") and L.met2_abi_version() == 6


def test_invert_runs_the_loop_with_a_host_step(warp, smooth):
    u, A, inv = smooth
    out = warp.invert(u, A, wi.SMOOTH_DST, n_iter=30, step=wi.STEP)
    assert set(out) == {"disp", "B", "inside", "residual"}
    assert out["disp"].shape == wi.SMOOTH_DST + (3,) and out["disp"].dtype == np.float64 and out["inside"].dtype == np.uint8
    assert np.array_equal(out["disp"], inv[np.float64]["disp"]) and np.array_equal(out["residual"], inv[np.float64]["residual"])
    assert np.array_equal(out["inside"], inv[np.float64]["inside"]) and np.allclose(out["B"], inv[np.float64]["B"], rtol=0, atol=1e-15)
    none = warp.invert(u, A, wi.SMOOTH_DST, n_iter=0, step=wi.STEP)
    assert not none["disp"].any() and none["residual"].shape == (0,) and none["inside"] is None


def test_python_refusals(warp):
    filters = importlib.import_module(PKG + ".filters")
    motor = importlib.import_module(PKG + ".motor")
    u, A = wi.smooth_field(), wi.smooth_transform()
    B, N = wi.inverse_matrices(A)
    singular = A.copy()
    singular[:, 0] = 0.0
    bad_B = B.copy()
    bad_B[0, 0] = np.nan
    res = {k: np.zeros(wi.GRID) for k in filters.STAT_QUANTITIES}
    calls = ((lambda: warp.invert(u[..., :2], A, wi.SMOOTH_DST, step=wi.STEP), "disp"), (lambda: warp.invert(u, singular, wi.SMOOTH_DST, step=wi.STEP), "singular"),
             (lambda: warp.invert(u, A, (22, 17), step=wi.STEP), "grid"), (lambda: warp.invert(u, A, (22, 17, 513), step=wi.STEP), "512"),
             (lambda: warp.invert(u, A, wi.SMOOTH_DST, n_iter=-1, step=wi.STEP), "n_iter"), (lambda: warp.invert(u, A, wi.SMOOTH_DST, n_iter=2.5, step=wi.STEP), "n_iter"),
             (lambda: warp.invert(u, A, wi.SMOOTH_DST, step=3), "callable"), (lambda: warp.invert_step(u, bad_B, N, wi.SMOOTH_DST), "3 x 4"),
             (lambda: warp.invert_step(u, B, N[:2], wi.SMOOTH_DST), "3 x 3"), (lambda: warp.invert_step(u, B, np.full((3, 3), np.inf), wi.SMOOTH_DST), "3 x 3"),
             (lambda: warp.invert_step(u, B, N, wi.SMOOTH_DST, v_in=u), "v_in"), (lambda: warp.invert_step(u, B, N, wi.SMOOTH_DST, res2=np.zeros(1)), "res2"),
             (lambda: warp.jacobian(u[..., 0]), "disp"), (lambda: warp.jacobian(u, scale=np.nan), "scale"),
             (lambda: filters.maps_to_template_filter(res, np.eye(4), wi.SMOOTH_DST, np.eye(4), disp=u[:-1]), "disp"),
             (lambda: filters.maps_to_template_filter(res, np.eye(4), wi.SMOOTH_DST, np.eye(4), disp=u, order=3), "order"),
             (lambda: motor.motor_maps_to_template("x/", "t.nii.gz", path_to_world="w.txt", register={}), "path_to_world"),
             (lambda: motor.motor_maps_to_template("x/", "t.nii.gz", path_to_world="w.txt", nonlinear=True), "path_to_world"),
             (lambda: motor.motor_maps_to_template("x/", "t.nii.gz", path_to_warp="f.nii.gz", nonlinear=True), "path_to_warp"),
             (lambda: motor.motor_maps_to_template("x/", "t.nii.gz", nonlinear=3), "nonlinear"))
    for call, match in calls:
        with pytest.raises(ValueError, match=match):
            call()
    assert motor.maps_to_template_filter is filters.maps_to_template_filter and motor.warp_invert_filter is filters.warp_invert_filter
    assert motor.warp_jacobian_filter is filters.warp_jacobian_filter
