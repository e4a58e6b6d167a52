"""met2_warp_invert_step and met2_warp_jacobian on the device (include/met2_hip.h states the contract) against their numpy restatement in
long double (tests/tools/warp_inverse_numpy.py), the loop of warp.invert with device steps, and the maps brought onto a template's grid end to
end (maps_to_template_filter, motor_maps_to_template).
Bounds.  What the contract fixes in fp64 must be EQUAL: `inside`, n_nonpositive, and res2 against the rule evaluated in numpy on the device's
own v_out (a maximum does not depend on the order).  Every other quantity q is held to max |device - long double| / max |long double| <= 16 x
the largest such figure measured on an MI355X over these very cases (profiles/warp_inverse_parity.json, per quantity: invert_step, jacobian,
invert_25_steps), which may not exceed 1e-12: a larger error would be a defect, not rounding.  With MET2_WARP_INVERSE_PARITY_OUT=<file> the
module writes what it measured there.
Grids: warp_numpy.GRIDS -- 1 x 1 x 1 (every difference is 0), 9 x 1 x 4 (an axis of length 1), 7 x 5 x 3 (rims everywhere), 20 x 18 x 16 (the
smooth-field case), 17 x 17 x 257 (one voxel past a block of 256 along z, and 291 blocks for the maximum and the count across blocks) -- and
2 x 3 x 2 for the Jacobian (rims only).  The parity inputs keep every coordinate 1e-9 away from an integer and from a face (asserted), so a
rounding cannot move a tap or `inside`.
The label round trip: warp_numpy.atlas_case()'s labels pushed onto the maps through (A, u) and pulled back through (B, v) agree with the
originals in at least the share the restatement reaches on the CPU (profiles/warp_inverse_recovery.json: 0.9767 of 515 labelled voxels)
minus 0.5 % of the labelled voxels for ties at label borders."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import register_numpy as gn                                        # noqa: E402
import warp_numpy as wn                                            # noqa: E402
import warp_inverse_numpy as wi                                    # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
CEILING = 1e-12
QUANTITIES = ("invert_step", "jacobian", "invert_25_steps")
MEASURED = {q: 0.0 for q in QUANTITIES}
INVALID = -1                                                       # MET2_E_INVALID
LD = np.longdouble


def _json(name):
    path = os.path.join(ROOT, "profiles", name)
    assert os.path.exists(path), "%s is missing: it holds the measured figures the bounds derive from" % path
    return json.load(open(path))


def held(quantity, got, want):
    """records max |got - want| / max |want| for `quantity`, prints it, and holds it to the bound"""
    want = np.asarray(want, dtype=LD)
    den = np.abs(want).max() if want.size else LD(0)
    err = float(np.abs(np.asarray(got, dtype=LD) - want).max() / (den if den > 0 else LD(1))) if want.size else 0.0
    MEASURED[quantity] = max(MEASURED[quantity], err)
    print("%s: relative error %.3g" % (quantity, err))
    b = 16.0 * float(_json("warp_inverse_parity.json")["max_rel_error"][quantity])
    assert 0.0 < b <= CEILING, "the measured error of %s puts the bound at %g: above %g it is a defect, not rounding" % (quantity, b, CEILING)
    assert err <= b, (quantity, err, b)


@pytest.fixture(scope="module")
def warp():
    yield importlib.import_module(PKG + ".warp")
    path = os.environ.get("MET2_WARP_INVERSE_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"max_rel_error": MEASURED, "reference": "tests/tools/warp_inverse_numpy.py in long double",
                       "measure": "max |error| / max |reference| per call", "bound_factor": 16, "ceiling": CEILING,
                       "device": torch.cuda.get_device_name(0)}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib").lib()


@pytest.fixture(scope="module")
def smooth_25():
    """the smooth-field case after 25 steps in long double, computed once"""
    u, A = wi.smooth_field(), wi.smooth_transform()
    return u, A, wi.invert(u, A, wi.SMOOTH_DST, 25, LD)


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda").to(dtype).contiguous()


def step_case(grid):
    """u_src on the source grid of `grid`, the transform, a full N and a random v_in of amplitude 1"""
    src = wn.source_dims(grid)
    v_in = np.random.default_rng([11] + list(grid)).uniform(-1.0, 1.0, tuple(grid) + (3,))
    return src, wn.case_field(src), wn.case_transform(grid), wi.case_matrix(), v_in


# ---------------------------------------------------------------- met2_warp_invert_step

@pytest.mark.parametrize("grid", wn.GRIDS)
def test_step_parity(warp, grid):
    src, u, B, N, v_in = step_case(grid)
    for v in (v_in, None):
        want, want_in, _, c = wi.invert_step(u, B, N, grid, v, True, True, LD, True)
        assert wn.coordinate_margin(c, src) > wn.MARGIN
        got, got_in, got_r2 = warp.invert_step(u, B, N, grid, v_in=v, return_inside=True, return_res2=True)
        assert got.shape == tuple(grid) + (3,) and got_in.dtype == np.uint8 and np.array_equal(got_in, want_in)
        held("invert_step", got, want)
        assert got_r2 == float(wi.res2_of(got, v, np.float64)) and got_r2 > 0.0
        if v is not None and min(grid) > 1:
            assert 0 < want_in.sum() < want_in.size, "the case has voxels on either side of the inside test"
    # v_in = NULL gives the bits of v_in = zeros; tensors in, tensors out, the same bits; res2 into a caller's element
    zero = warp.invert_step(u, B, N, grid, v_in=np.zeros(tuple(grid) + (3,)), return_inside=True, return_res2=True)
    assert all(np.array_equal(a, b) for a, b in zip(zero, (got, got_in, got_r2)))
    row = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    t_out, t_in, t_r2 = warp.invert_step(dev(u), B, N, grid, v_in=dev(v_in), return_inside=True, return_res2=True, res2=row[1:2])
    first = warp.invert_step(u, B, N, grid, v_in=v_in, return_inside=True, return_res2=True)
    assert t_out.is_cuda and t_r2.data_ptr() == row[1:2].data_ptr() and row.cpu().tolist() == [-1.0, first[2], -1.0]
    assert np.array_equal(t_out.cpu().numpy(), first[0]) and np.array_equal(t_in.cpu().numpy(), first[1])
    assert np.array_equal(warp.invert_step(u, B, N, grid, v_in=v_in), first[0])            # no inside, no res2


@pytest.mark.parametrize("grid", wn.GRIDS)
def test_step_with_a_diagonal_N_is_met2_warp_compose(warp, grid):
    src, u, B, _, _ = step_case(grid)
    gain = (2.0, -1.5, 0.75)
    assert np.array_equal(warp.invert_step(u, B, np.diag(gain), grid), warp.compose(u, grid, B, gain))


def test_res2_passes_over_what_is_not_a_number_and_is_zero_for_no_change(warp):
    grid = (7, 5, 3)
    u = wn.case_field(grid)
    eye = wi.IDENTITY
    # N = identity, B = identity, v_in = u: v_out = u(clamp(y + u)); with u = 0 nothing changes
    zero = np.zeros(tuple(grid) + (3,))
    out, r2 = warp.invert_step(zero, eye, np.eye(3), grid, v_in=zero, return_res2=True)
    assert r2 == 0.0 and not out.any()
    u[3, 2, 1, 0] = np.nan                                         # a sample that is not a number: the voxels that take it are passed over
    got, r2 = warp.invert_step(u, eye, np.eye(3), grid, return_res2=True)
    assert np.isnan(got).any() and r2 == float(wi.res2_of(got, None, np.float64)) and np.isfinite(r2) and r2 > 0.0


# ---------------------------------------------------------------- the loop

def test_25_steps_on_the_smooth_field(warp, smooth_25):
    u, A, want = smooth_25
    out = warp.invert(u, A, wi.SMOOTH_DST, n_iter=25)
    assert set(out) == {"disp", "B", "inside", "residual"} and out["residual"].shape == (25,)
    assert np.allclose(out["B"], want["B"], rtol=0, atol=1e-15)
    held("invert_25_steps", out["disp"], want["disp"])
    print("residual: device %.6e, long double %.6e" % (out["residual"][-1], want["residual"][-1]))
    assert np.abs(out["residual"] - want["residual"]).max() <= 1e-9
    err, ins = wi.round_trip_error(u, A, out)
    bound = 2.0 * np.abs(A[:, :3]).sum(axis=1).max() * out["residual"][-1]
    print("invariant: %.3g <= %.3g over %.1f %% of the voxels" % (float(err[ins].max()), bound, 100 * ins.mean()))
    assert float(err[ins].max()) <= bound
    c = want["coords"]
    near = np.zeros(wi.SMOOTH_DST, dtype=bool)
    for a in range(3):
        near |= (np.abs(c[a]) <= 1e-9) | (np.abs(c[a] - (wi.GRID[a] - 1)) <= 1e-9)
    assert near.sum() <= 0.001 * near.size
    assert np.array_equal(out["inside"][~near], want["inside"][~near])
    again = warp.invert(u, A, wi.SMOOTH_DST, n_iter=25)
    assert all(np.array_equal(again[k], out[k]) for k in out)
    none = warp.invert(u, A, wi.SMOOTH_DST, n_iter=0)
    assert not none["disp"].any() and none["residual"].shape == (0,) and none["inside"] is None
    one = warp.invert(u, A, wi.SMOOTH_DST, n_iter=1)
    assert np.array_equal(one["disp"], warp.invert_step(u, out["B"], -A[:, :3], wi.SMOOTH_DST))


def test_linear_field_reaches_the_closed_form_on_the_device(warp):
    want, ok = wi.linear_inverse()
    out = warp.invert(wi.linear_field(), wi.IDENTITY, wi.GRID, n_iter=40)
    err = np.abs(out["disp"] - want)[ok].max()
    ratio = out["residual"][1:12] / out["residual"][:11]
    print("|v - closed form| = %.3g over %.1f %% of the voxels; residual ratios %s" % (err, 100 * ok.mean(), ratio))
    assert err <= 1e-12 and np.all((ratio > 0.09) & (ratio < 0.12))
    const = np.broadcast_to(wi.LINEAR_T, wi.GRID + (3,)).copy()
    two = warp.invert(const, wi.IDENTITY, wi.GRID, n_iter=2)
    assert np.array_equal(two["disp"], -const) and two["residual"][1] == 0.0
    assert two["residual"][0] == np.sqrt((0.5 * 0.5 + 0.25 * 0.25) + 0.125 * 0.125)


# ---------------------------------------------------------------- met2_warp_jacobian

@pytest.mark.parametrize("grid", wi.JACOBIAN_GRIDS)
def test_jacobian_parity(warp, grid):
    n = int(np.prod(grid))
    for u, scale in ((wn.case_field(grid), 1.0), (wn.case_field(grid, 0.4), -0.83), (wi.linear_field(grid), 1.0)):
        want, _ = wi.jacobian(u, scale, LD)
        det, count = warp.jacobian(u, scale)
        assert det.shape == tuple(grid) and isinstance(count, int)
        held("jacobian", det, want)
        assert count == int((~(det > 0)).sum()) == wi.jacobian(u, scale, np.float64)[1]
    one, count = warp.jacobian(np.zeros(tuple(grid) + (3,)), 1.0)
    assert np.array_equal(one, np.ones(grid)) and count == 0
    det, count = warp.jacobian(wi.folded_field(grid))
    assert (np.array_equal(det, np.full(grid, -0.5)) and count == n) if grid[0] > 1 else (np.array_equal(det, np.ones(grid)) and count == 0)
    t_det, t_count = warp.jacobian(dev(wi.folded_field(grid)))
    assert t_det.is_cuda and t_count.dtype == torch.int64 and int(t_count.cpu()[0]) == count and np.array_equal(t_det.cpu().numpy(), det)
    u = wn.case_field(grid)
    u[0, 0, 0, 1] = np.nan
    det, count = warp.jacobian(u)
    assert count == int((~(det > 0)).sum()) and (np.isnan(det[0, 0, 0]) if max(grid) > 1 else det[0, 0, 0] == 1.0)


def test_jacobian_counts_folds_across_block_seams(warp):
    u, folds = wi.designed_folds()
    det, count = warp.jacobian(u)
    assert count == folds.size and np.array_equal(np.flatnonzero(~(det.reshape(-1) > 0)), folds)
    filters = importlib.import_module(PKG + ".filters")
    det2, count2 = filters.warp_jacobian_filter(u, scale=2.0)
    assert count2 == count and np.array_equal(det2, 2.0 * det)


# ---------------------------------------------------------------- the refusals

def test_every_refusal_leaves_the_outputs_untouched(L):
    grid = (7, 5, 3)
    src, u, B, N, v_in = step_case(grid)
    i3 = lambda d: (C.c_int32 * 3)(*d)
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    bad_B, bad_N = B.copy(), N.copy()
    bad_B[2, 1] = np.nan
    bad_N[1, 1] = np.nan
    n = int(np.prod(grid))
    du, dv = dev(u), dev(v_in)
    keep_u, keep_v = du.clone(), dv.clone()
    out = torch.full((n * 3,), 12345.0, dtype=torch.float64, device="cuda")
    out_b = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    r2 = torch.full((1,), 777.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((1,), 55, dtype=torch.int64, device="cuda")
    o, b, r, p = out.data_ptr(), out_b.data_ptr(), r2.data_ptr(), None
    calls = [
        L.met2_warp_invert_step(0, i3(src), p, i3(grid), dp(B), dp(N), dv.data_ptr(), o, b, r, None),                   # NULL u
        L.met2_warp_invert_step(0, i3(src), du.data_ptr(), i3(grid), dp(B), dp(N), dv.data_ptr(), p, b, r, None),       # NULL v_out
        L.met2_warp_invert_step(0, i3(src), du.data_ptr(), i3((7, 0, 3)), dp(B), dp(N), dv.data_ptr(), o, b, r, None),  # an axis of 0
        L.met2_warp_invert_step(0, i3((0, 6, 4)), du.data_ptr(), i3(grid), dp(B), dp(N), dv.data_ptr(), o, b, r, None),
        L.met2_warp_invert_step(0, i3(src), du.data_ptr(), i3(grid), dp(bad_B), dp(N), dv.data_ptr(), o, b, r, None),   # a NaN in B
        L.met2_warp_invert_step(0, i3(src), du.data_ptr(), i3(grid), dp(B), dp(bad_N), dv.data_ptr(), o, b, r, None),   # a NaN in N
        L.met2_warp_invert_step(0, i3(src), du.data_ptr(), i3(grid), dp(B), None, dv.data_ptr(), o, b, r, None),
        L.met2_warp_invert_step(0, i3(src), du.data_ptr(), i3(grid), dp(B), dp(N), dv.data_ptr(), dv.data_ptr(), b, r, None),   # v_out == v_in
        L.met2_warp_invert_step(0, i3(src), du.data_ptr(), i3(grid), dp(B), dp(N), dv.data_ptr(), du.data_ptr(), b, r, None),   # v_out == u_src
        L.met2_warp_jacobian(0, i3(grid), p, 1.0, o, cnt.data_ptr(), None),
        L.met2_warp_jacobian(0, i3(grid), dv.data_ptr(), 1.0, p, cnt.data_ptr(), None),
        L.met2_warp_jacobian(0, i3((7, 5, 0)), dv.data_ptr(), 1.0, o, cnt.data_ptr(), None),
        L.met2_warp_jacobian(0, i3(grid), dv.data_ptr(), float("nan"), o, cnt.data_ptr(), None),
        L.met2_warp_jacobian(0, i3(grid), dv.data_ptr(), 1.0, dv.data_ptr(), cnt.data_ptr(), None),                      # det == u
    ]
    torch.cuda.synchronize()
    assert calls == [INVALID] * len(calls), calls
    assert bool((out == 12345.0).all()) and bool((out_b == 9).all()) and float(r2.cpu()[0]) == 777.0 and int(cnt.cpu()[0]) == 55
    assert torch.equal(du, keep_u) and torch.equal(dv, keep_v)
    big = [L.met2_warp_invert_step(0, i3((513, 2, 2)), du.data_ptr(), i3(grid), dp(B), dp(N), p, o, b, r, None),
           L.met2_warp_invert_step(0, i3(src), du.data_ptr(), i3((2, 513, 2)), dp(B), dp(N), p, o, b, r, None),
           L.met2_warp_jacobian(0, i3((2, 2, 513)), dv.data_ptr(), 1.0, o, cnt.data_ptr(), None)]
    torch.cuda.synchronize()
    assert big == [-2] * 3 and bool((out == 12345.0).all()) and float(r2.cpu()[0]) == 777.0 and int(cnt.cpu()[0]) == 55     # MET2_E_UNSUPPORTED


# ---------------------------------------------------------------- end to end

def maps_case(motor):
    fixed, moving, aff = wn.recovery_pair()
    rng = np.random.default_rng(8)
    res = {k: rng.random(gn.PHANTOM_SHAPE) for k in motor.STAT_QUANTITIES}
    res["TWC"] = fixed                                             # the reference volume the template is registered to
    return res, aff, moving


def test_maps_to_template_filter(warp):
    motor = importlib.import_module(PKG + ".motor")
    rs = importlib.import_module(PKG + ".resample")
    lab, la, fa, A, u, truth = wi.round_trip_inputs()
    res, aff, _ = maps_case(motor)
    assert np.array_equal(aff, fa)
    # without a field: resample_filter with the inverse matrix, to the bit
    plain = motor.maps_to_template_filter(res, fa, lab.shape, la, order=1)
    B = np.ascontiguousarray(rs.invert(rs.voxel_matrix(fa, la))[:3])
    for k in motor.STAT_QUANTITIES:
        want, want_in = motor.resample_filter(res[k], B, lab.shape, order=1, cval=0.0, return_inside=True)
        assert np.array_equal(plain[k], want) and np.array_equal(plain["inside"], want_in)
    assert plain["inverse_disp"] is None and plain["jacobian"] is None and plain["residual"].shape == (0,) and plain["n_nonpositive"] == 0
    assert 0 < plain["inside"].sum() < plain["inside"].size and not plain["MWF"][plain["inside"] == 0].any()
    # the labels, pushed onto the maps through (A, u), come back through (B, v)
    res["MWF"] = truth.astype(np.float64)
    out = motor.maps_to_template_filter(res, fa, lab.shape, la, disp=u, order=0, n_iter=20)
    share, n_lab = wi.label_share(out["MWF"], lab)
    rec = _json("warp_inverse_recovery.json")
    print("labels recovered: %.4f of %d (the restatement: %.4f); last residual %.3g" % (share, n_lab, rec["share_recovered"], out["residual"][-1]))
    assert n_lab == rec["n_labelled"] and share >= rec["share_recovered"] - rec["margin_share"]
    assert out["inverse_disp"].shape == lab.shape + (3,) and out["residual"].shape == (20,) and out["residual"][-1] < 1e-5
    assert out["jacobian"].shape == gn.PHANTOM_SHAPE and out["n_nonpositive"] == 0 and 0.9 < out["jacobian"].min() < out["jacobian"].max() < 1.2
    inv = motor.warp_invert_filter(u, A, lab.shape, n_iter=20)
    assert np.array_equal(inv["disp"], out["inverse_disp"]) and np.array_equal(inv["residual"], out["residual"])
    back = motor.warp_labels_filter(truth, inv["B"], inv["disp"], fill=0)
    assert np.array_equal(back, out["MWF"].astype(np.int32))


def test_motor_maps_to_template(warp, tmp_path):
    motor = importlib.import_module(PKG + ".motor")
    nifti = importlib.import_module(PKG + ".nifti")
    res, aff, template = maps_case(motor)
    tpl_aff = aff.copy()
    tpl_aff[:3, 3] += (1.0, -2.0, 1.5)
    tpl_shape = (22, 19, 17)
    tpl = np.zeros(tpl_shape)
    tpl[:20, :18, :16] = template
    out = str(tmp_path) + os.sep
    for k in motor.STAT_QUANTITIES:
        nifti.save(nifti.NiftiImage(res[k], aff), out + k + ".nii.gz")
    nifti.save(nifti.NiftiImage(tpl, tpl_aff), out + "template.nii.gz")
    before = set(os.listdir(out))
    got = motor.motor_maps_to_template(out, out + "template.nii.gz", nonlinear={"iters": (0, 10, 5)}, n_iter=20)
    new = {k + "_in_template.nii.gz" for k in motor.STAT_QUANTITIES} | {"maps_to_template_warp.nii.gz", "maps_to_template_inside.nii.gz",
                                                                        "template_to_maps_jacobian.nii.gz", "maps_to_template_report.txt"}
    assert set(os.listdir(out)) == before | new
    for k in motor.STAT_QUANTITIES:
        img = nifti.load(out + k + "_in_template.nii.gz")
        assert img.get_fdata().shape == tpl_shape and np.allclose(img.affine, tpl_aff) and np.array_equal(img.get_fdata(), got[k])
    field = nifti.load(out + "maps_to_template_warp.nii.gz")
    assert field.get_fdata().shape == tpl_shape + (3,) and np.allclose(field.affine, tpl_aff) and np.array_equal(field.get_fdata(), got["inverse_disp"])
    ins = nifti.load(out + "maps_to_template_inside.nii.gz")
    assert ins.get_fdata().shape == tpl_shape and np.allclose(ins.affine, tpl_aff) and np.array_equal(ins.get_fdata(), got["inside"])
    jac = nifti.load(out + "template_to_maps_jacobian.nii.gz")
    assert jac.get_fdata().shape == gn.PHANTOM_SHAPE and np.allclose(jac.affine, aff) and np.array_equal(jac.get_fdata(), got["jacobian"])
    report = open(out + "maps_to_template_report.txt").read().splitlines()
    assert len([l for l in report if l.startswith("step ")]) == 20 and any("not positive" in l for l in report) and any("min" in l and "max" in l for l in report)
    assert got["disp"].shape == gn.PHANTOM_SHAPE + (3,) and got["residual"].shape == (20,) and got["world"].shape == (4, 4)
    # the matrix and the field of that run, given as files, reproduce its maps
    np.savetxt(out + "world.txt", got["world"])
    nifti.save(nifti.NiftiImage(got["disp"], aff), out + "field.nii.gz")
    again = motor.motor_maps_to_template(out, out + "template.nii.gz", path_to_world=out + "world.txt", path_to_warp=out + "field.nii.gz", n_iter=20)
    for k in motor.STAT_QUANTITIES + ("inside", "inverse_disp", "jacobian", "residual"):
        assert np.array_equal(again[k], got[k]), k
    # a matrix alone: no field, no inverse, no Jacobian
    for f in new:
        os.remove(out + f)
    plain = motor.motor_maps_to_template(out, out + "template.nii.gz", path_to_world=out + "world.txt")
    assert plain["inverse_disp"] is None and plain["disp"] is None
    assert set(os.listdir(out)) == (before | new | {"world.txt", "field.nii.gz"}) - {"maps_to_template_warp.nii.gz", "template_to_maps_jacobian.nii.gz"}
    for call, match in ((lambda: motor.motor_maps_to_template(out, out + "template.nii.gz", path_to_world=out + "world.txt", nonlinear=True), "path_to_world"),
                        (lambda: motor.motor_maps_to_template(out, out + "template.nii.gz", path_to_world=out + "world.txt", register={"dof": 6}), "path_to_world"),
                        (lambda: motor.motor_maps_to_template(out, out + "template.nii.gz", path_to_warp=out + "field.nii.gz", nonlinear=True), "path_to_warp"),
                        (lambda: motor.motor_maps_to_template(out, out + "template.nii.gz", path_to_world=out + "world.txt", path_to_warp=out + "MWF.nii.gz"), "field")):
        with pytest.raises(ValueError, match=match):
            call()
