"""The displacement-field entries on the device (met2_warp, met2_warp_labels, met2_warp_compose, met2_warp_max_norm2, met2_warp_lncc and its
stage entries; include/met2_hip.h states the contract) against their numpy restatement in long double (tests/tools/warp_numpy.py), and the
non-linear registration end to end with device stages.
Bounds.  What the contract fixes in fp64 -- coordinates, inside, taps, order 0, labels, the count n, the largest norm -- must be EQUAL.  Every
other quantity q is held to max |device - long double| / max |long double| <= 16 x the largest such figure measured on an MI355X over these
very cases (profiles/warp_parity.json, per quantity: head-room for another rounding order on another device), which may not exceed 1e-12: a
larger error would be a defect, not rounding.  With MET2_WARP_PARITY_OUT=<file> the module writes what it measured there.
Grids (warp_numpy.GRIDS): 1 x 1 x 1, 9 x 1 x 4, 7 x 5 x 3, the phantom's 20 x 18 x 16, and 17 x 17 x 257: one voxel past a thread's segment of 16
outputs on x and y and past the z pass' tile of 256.  Radii 1, 2 and 4, wider than an axis on the small grids.  The parity cases keep every
coordinate 1e-9 away from an integer, a half and a face (asserted; tests/test_warp_host.py asserts the same without a device), so a rounding
cannot move a tap.
End to end: the recovery case of tests/test_warp_host.py with device stages meets that test's bound (error after <= 0.65 x before, the last
metric above the first) and ends within 0.1 mm -- a twentieth of a voxel, far below what moves a label -- of the restatement's error in
profiles/warp_recovery.json: the two take different rounding paths over 45 iterations, so equal fields are not asked for."""
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
import resample_numpy as rn                                        # noqa: E402
import warp_numpy as wn                                            # noqa: E402

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
CEILING = 1e-12
QUANTITIES = ("warp_order1", "compose", "lncc_sums", "lncc_force", "lncc_metric")
MEASURED = {q: 0.0 for q in QUANTITIES}
E2E_MARGIN_MM = 0.1
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
    b = 16.0 * float(_json("warp_parity.json")["max_rel_error"][quantity])
    assert 0.0 < b <= CEILING, "the measured error of %s puts the bound at %g: above %g it is a defect, not rounding" % (quantity, b, CEILING)
    assert err <= b, (quantity, err, b)


@pytest.fixture(scope="module")
def warp():
    yield importlib.import_module(PKG + ".warp")
    path = os.environ.get("MET2_WARP_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"max_rel_error": MEASURED, "reference": "tests/tools/warp_numpy.py in long double", "measure": "max |error| / max |reference| per call",
                       "bound_factor": 16, "ceiling": CEILING, "device": torch.cuda.get_device_name(0)}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def resample():
    return importlib.import_module(PKG + ".resample")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib").lib()


def dev(x, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda").to(dtype).contiguous()


# ---------------------------------------------------------------- met2_warp, met2_warp_labels

@pytest.mark.parametrize("grid", wn.GRIDS)
def test_a_zero_field_is_met2_resample_to_the_bit(warp, resample, grid):
    src = wn.source_dims(grid)
    vol = wn.case_volume(grid, 3)
    zero = np.zeros(tuple(grid) + (3,))
    for name in ("rotated", "half"):
        A = rn.transforms(src, grid)[name]
        for order in (0, 1):
            for layout, v in (("series", vol), ("voxel", np.ascontiguousarray(np.moveaxis(vol, 0, 3)))):
                want, want_in = resample.resample(v, A, grid, order=order, cval=-7.0, layout=layout, return_inside=True)
                got, got_in = warp.warp(v, A, zero, order=order, cval=-7.0, layout=layout, return_inside=True)
                assert np.array_equal(got_in, want_in) and np.array_equal(got, want), (name, order, layout)
    lab = wn.case_labels(grid)
    assert np.array_equal(warp.warp_labels(lab, A, zero, fill=-1), resample.resample_labels(lab, A, grid, fill=-1))


@pytest.mark.parametrize("grid", wn.GRIDS)
def test_warp_through_a_smooth_field(warp, grid):
    src, A, u, vol = wn.source_dims(grid), wn.case_transform(grid), wn.case_field(grid), wn.case_volume(grid, 2)
    want1, want_in, c = wn.warp(vol, A, u, 1, 2.5, LD, return_inside=True, return_coords=True)
    assert wn.coordinate_margin(c, src) > wn.MARGIN
    if grid == gn.PHANTOM_SHAPE:
        assert 0 < want_in.sum() < want_in.size and np.abs(u).max() > 2.9
    got1, got_in = warp.warp(vol, A, u, order=1, cval=2.5, return_inside=True)
    assert np.array_equal(got_in, want_in)
    got0 = warp.warp(vol, A, u, order=0, cval=2.5)
    assert np.array_equal(got0, wn.warp(vol, A, u, 0, 2.5))
    assert np.array_equal(got1[:, want_in == 0], np.full((2, int((want_in == 0).sum())), 2.5))
    held("warp_order1", got1, want1)
    # voxel-major series give the same bits, and so does a second call
    vm = warp.warp(np.ascontiguousarray(np.moveaxis(vol, 0, 3)), A, u, order=1, cval=2.5, layout="voxel")
    assert np.array_equal(np.moveaxis(vm, 3, 0), got1) and np.array_equal(warp.warp(vol, A, u, order=1, cval=2.5), got1)
    lab = wn.case_labels(grid)
    got_lab, lab_in = warp.warp_labels(lab, A, u, fill=-9, return_inside=True)
    assert got_lab.dtype == np.int32 and np.array_equal(got_lab, wn.warp_labels(lab, A, u, fill=-9)) and np.array_equal(lab_in, want_in)


# ---------------------------------------------------------------- met2_warp_compose, met2_warp_max_norm2

@pytest.mark.parametrize("grid", wn.GRIDS)
def test_compose(warp, grid):
    u = wn.case_field(grid)
    eye = np.column_stack([np.eye(3), np.zeros(3)])
    # the identity: every coordinate an integer, weights 1 and 0
    assert np.array_equal(warp.compose(u, grid), u)
    assert np.array_equal(warp.compose(u, grid, eye, (1.0, 1.0, 1.0), np.ones(tuple(grid) + (3,)), 0.25, 0.0), u)      # *vmax2 = 0: s = 0
    # an update of up to 3 voxels: phi o (id + w), coordinates beyond the rim clamped
    v = wn.case_field(grid, 40.0)[..., ::-1].copy()
    m2 = wn.max_norm2(v)
    want, c_raw = wn.compose(u, grid, eye, (1.0, 1.0, 1.0), v, 3.0, m2, LD, return_coords=True)
    if min(grid) > 1:
        assert any((c_raw[a] < 0).any() or (c_raw[a] > grid[a] - 1).any() for a in range(3)), "no coordinate is clamped"
    held("compose", warp.compose(u, grid, eye, (1.0, 1.0, 1.0), v, 3.0, m2), want)
    on_device = warp.compose(dev(u), grid, eye, (1.0, 1.0, 1.0), dev(v), 3.0, warp.max_norm2(dev(v)))
    assert np.array_equal(on_device.cpu().numpy(), warp.compose(u, grid, eye, (1.0, 1.0, 1.0), v, 3.0, m2))
    # a change of grid: no update, a matrix between the grids, gains that are not 1; the finer grid reaches past the coarse one's rim
    fine = tuple(min(2 * n + 1, 512) for n in grid)                 # 512: the longest axis the entries take
    A = np.column_stack([np.diag([0.5, 0.5, 0.5]), [-0.3, -0.2, -0.4]])
    gain = (2.0, 1.5, 0.75)
    want, c_raw = wn.compose(u, fine, A, gain, None, 0.0, None, LD, return_coords=True)
    assert (c_raw < 0).any()
    held("compose", warp.compose(u, fine, A, gain), want)
    # step alone (vmax2 = None): w = step v
    held("compose", warp.compose(u, grid, eye, (1.0, 1.0, 1.0), v, 0.01), wn.compose(u, grid, eye, (1.0, 1.0, 1.0), v, 0.01, None, LD))


@pytest.mark.parametrize("shape", wn.GRIDS + ((64, 64, 70),))
def test_max_norm2_is_exact(warp, shape):
    # 64 x 64 x 70 = 286 720 voxels: more than the 1 024 blocks of 256 the launch is capped at
    v = np.random.default_rng(list(shape)).standard_normal(tuple(shape) + (3,)) * 3.0
    assert warp.max_norm2(v) == wn.max_norm2(v)
    assert warp.max_norm2(np.zeros(tuple(shape) + (3,))) == 0.0
    v[-1, -1, -1] = (100.0, -3.0, 0.5)                             # the last voxel holds the maximum
    assert warp.max_norm2(v) == wn.max_norm2(v) == (100.0 * 100.0 + 9.0) + 0.25


# ---------------------------------------------------------------- met2_warp_lncc

@pytest.mark.parametrize("grid", wn.GRIDS)
def test_lncc_sums_force_and_metric(warp, L, grid):
    F, W, m = wn.lncc_inputs(grid)
    for r in wn.RADII:
        want = wn.lncc_sums(F, W, m, r, LD)
        sums = warp.lncc_sums(F, W, m, r)
        assert np.array_equal(sums[0], want[0].astype(np.float64)), "n must be exact"
        for c in range(1, 6):
            if np.abs(want[c]).max() > 0:
                held("lncc_sums", sums[c], want[c])
        # the force from the device's own sums
        wf, (wcc, wn_valid), valid, (B, Cc) = wn.lncc_force(F, W, m, sums, wn.FORCE_EPS, LD, return_terms=True)
        assert wn.eps_margin(B, Cc, m, sums[0], wn.FORCE_EPS)
        force, metric = warp.lncc_force(F, W, m, sums, wn.FORCE_EPS)
        assert metric[1] == wn_valid and not force[~valid].any()
        if wn_valid:
            held("lncc_force", force, wf)
            held("lncc_metric", metric[0], wcc)
        else:
            assert not force.any() and metric[0] == 0.0
        # the whole entry: the same bits as its stages, from call to call, with a caller's work block and with its own
        f2, m2 = warp.lncc(F, W, m, r, wn.FORCE_EPS)
        f3, m3 = warp.lncc(F, W, m, r, wn.FORCE_EPS, work=torch.full(((warp.work_bytes(grid) + 7) // 8,), float("nan"), dtype=torch.float64, device="cuda"))
        assert np.array_equal(f2, force) and np.array_equal(m2, metric) and np.array_equal(f3, force) and np.array_equal(m3, metric)
    own_f, own_m = torch.empty(tuple(grid) + (3,), dtype=torch.float64, device="cuda"), torch.empty(2, dtype=torch.float64, device="cuda")
    dF, dW, dm = dev(F), dev(W), dev(m, torch.uint8)
    rc = L.met2_warp_lncc(0, (C.c_int32 * 3)(*grid), dF.data_ptr(), dW.data_ptr(), dm.data_ptr(), wn.RADII[-1], wn.FORCE_EPS, own_f.data_ptr(),
                          own_m.data_ptr(), None, 0, None)                  # no work block: the entry allocates its own and waits
    assert rc == 0 and np.array_equal(own_f.cpu().numpy(), force) and np.array_equal(own_m.cpu().numpy(), metric)


def test_work_bytes_and_the_python_refusals(warp):
    n6 = 6 * 20 * 18 * 16 * 8
    assert warp.work_bytes((20, 18, 16)) == 2 * ((n6 + 255) // 256 * 256) + 2 * 1024 * 8
    F, W, m = wn.lncc_inputs((7, 5, 3))
    u = wn.case_field((7, 5, 3))
    for call, match in ((lambda: warp.lncc(F, W, m, 0), "radius"), (lambda: warp.lncc(F, W, m, 5), "radius"), (lambda: warp.lncc(F, W, m, 2, -1.0), "eps"),
                        (lambda: warp.lncc(F, W[:-1], m, 2), "one shape"), (lambda: warp.warp(F, np.eye(4)[:3], u, order=3), "order"),
                        (lambda: warp.warp(F, np.eye(4)[:3], u[..., :2]), "disp"), (lambda: warp.compose(u, (7, 5, 3), gain=(1.0, np.nan, 1.0)), "gain"),
                        (lambda: warp.compose(u, (7, 5, 3), step=np.inf), "step"), (lambda: warp.warp_labels(F, np.eye(4)[:3], u), "integer")):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(importlib.import_module(PKG + "._lib").Met2Error, match="work block"):
        warp.lncc(F, W, m, 2, work=torch.empty(8, dtype=torch.float64, device="cuda"))


def test_every_refusal_leaves_the_outputs_untouched(L):
    grid = (7, 5, 3)
    src = wn.source_dims(grid)
    i3 = lambda d: (C.c_int32 * 3)(*d)
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    A, bad_A = wn.case_transform(grid), wn.case_transform(grid)
    bad_A[1, 2] = np.nan
    vol, lab, u = dev(wn.case_volume(grid, 1)[0]), dev(wn.case_labels(grid), torch.int32), dev(wn.case_field(grid))
    F, W, m = [dev(x, t) for x, t in zip(wn.lncc_inputs(grid), (torch.float64, torch.float64, torch.uint8))]
    n = int(np.prod(grid))
    out = torch.full((n * 6,), 12345.0, dtype=torch.float64, device="cuda")     # every double output points here
    out_i = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    out_b = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    work = torch.empty(16384, dtype=torch.float64, device="cuda")
    one = dev(np.ones(1))
    o, p = out.data_ptr(), None
    ok_gain, nan_gain = dp([1.0, 1.0, 1.0]), dp([1.0, np.inf, 1.0])
    calls = [
        L.met2_warp(0, 1, i3(src), 1, vol.data_ptr(), 1, 1, i3(grid), dp(A), p, 0.0, o, 1, 1, out_b.data_ptr(), None),                 # no field
        L.met2_warp(0, 3, i3(src), 1, vol.data_ptr(), 1, 1, i3(grid), dp(A), u.data_ptr(), 0.0, o, 1, 1, out_b.data_ptr(), None),      # order 3
        L.met2_warp(0, 1, i3(src), 1, vol.data_ptr(), 1, 1, i3(grid), dp(bad_A), u.data_ptr(), 0.0, o, 1, 1, out_b.data_ptr(), None),
        L.met2_warp(0, 1, i3(src), 1, p, 1, 1, i3(grid), dp(A), u.data_ptr(), 0.0, o, 1, 1, out_b.data_ptr(), None),
        L.met2_warp(0, 1, i3(src), 1, vol.data_ptr(), 0, 1, i3(grid), dp(A), u.data_ptr(), 0.0, o, 1, 1, out_b.data_ptr(), None),      # a stride of 0
        L.met2_warp(0, 1, i3((0, 5, 3)), 1, vol.data_ptr(), 1, 1, i3(grid), dp(A), u.data_ptr(), 0.0, o, 1, 1, out_b.data_ptr(), None),
        L.met2_warp(0, 1, i3(src), 2, vol.data_ptr(), 1, 1, i3(grid), dp(A), u.data_ptr(), 0.0, o, 1, 1, out_b.data_ptr(), None),      # two series share elements
        L.met2_warp_labels(0, i3(src), lab.data_ptr(), i3(grid), dp(A), p, 0, out_i.data_ptr(), out_b.data_ptr(), None),
        L.met2_warp_labels(0, i3(src), lab.data_ptr(), i3(grid), dp(bad_A), u.data_ptr(), 0, out_i.data_ptr(), out_b.data_ptr(), None),
        L.met2_warp_compose(0, i3(grid), u.data_ptr(), i3(grid), dp(A), nan_gain, p, 1.0, p, o, None),
        L.met2_warp_compose(0, i3(grid), u.data_ptr(), i3(grid), dp(A), ok_gain, p, float("inf"), p, o, None),
        L.met2_warp_compose(0, i3(grid), u.data_ptr(), i3(grid), dp(bad_A), ok_gain, p, 1.0, p, o, None),
        L.met2_warp_compose(0, i3(grid), p, i3(grid), dp(A), ok_gain, p, 1.0, p, o, None),
        L.met2_warp_compose(0, i3(grid), u.data_ptr(), i3(grid), dp(A), None, p, 1.0, p, o, None),
        L.met2_warp_max_norm2(0, n, p, o, None),
        L.met2_warp_max_norm2(0, 0, u.data_ptr(), o, None),
        L.met2_warp_lncc(0, i3(grid), F.data_ptr(), W.data_ptr(), m.data_ptr(), 0, 1e-10, o, o, work.data_ptr(), work.numel() * 8, None),
        L.met2_warp_lncc(0, i3(grid), F.data_ptr(), W.data_ptr(), m.data_ptr(), 5, 1e-10, o, o, work.data_ptr(), work.numel() * 8, None),
        L.met2_warp_lncc(0, i3(grid), F.data_ptr(), W.data_ptr(), m.data_ptr(), 2, -1e-10, o, o, work.data_ptr(), work.numel() * 8, None),
        L.met2_warp_lncc(0, i3(grid), F.data_ptr(), W.data_ptr(), m.data_ptr(), 2, float("nan"), o, o, work.data_ptr(), work.numel() * 8, None),
        L.met2_warp_lncc(0, i3(grid), F.data_ptr(), W.data_ptr(), p, 2, 1e-10, o, o, work.data_ptr(), work.numel() * 8, None),
        L.met2_warp_lncc(0, i3(grid), F.data_ptr(), W.data_ptr(), m.data_ptr(), 2, 1e-10, o, o, work.data_ptr(), 64, None),            # too small a block
        L.met2_warp_lncc_sums(0, i3(grid), F.data_ptr(), W.data_ptr(), m.data_ptr(), 7, o, work.data_ptr(), work.numel() * 8, None),
        L.met2_warp_lncc_sums(0, i3(grid), F.data_ptr(), p, m.data_ptr(), 2, o, work.data_ptr(), work.numel() * 8, None),
        L.met2_warp_lncc_force(0, i3(grid), F.data_ptr(), W.data_ptr(), m.data_ptr(), one.data_ptr(), -1.0, o, o, work.data_ptr(), work.numel() * 8, None),
        L.met2_warp_lncc_force(0, i3(grid), F.data_ptr(), W.data_ptr(), m.data_ptr(), p, 1e-10, o, o, work.data_ptr(), work.numel() * 8, None),
    ]
    torch.cuda.synchronize()
    assert calls == [INVALID] * len(calls), calls
    assert bool((out == 12345.0).all()) and bool((out_i == 77).all()) and bool((out_b == 9).all())
    big = (C.c_int32 * 3)(513, 2, 2)
    assert L.met2_warp_work_bytes(big, C.byref(C.c_int64())) == -2 and L.met2_warp_work_bytes(i3(grid), None) == INVALID


# ---------------------------------------------------------------- end to end

def recorded(inverted):
    return _json("warp_recovery.json")["inverted" if inverted else "same_contrast"]


@pytest.mark.parametrize("inverted", (False, True))
def test_recovery_with_device_stages(warp, inverted):
    fixed, moving, aff = wn.recovery_pair(inverted)
    out = warp.register(fixed, aff, moving, aff, None, **wn.RECOVERY_OPTIONS)
    before = wn.recovery_error(np.zeros(fixed.shape + (3,)), fixed, aff)
    after = wn.recovery_error(out["disp"], fixed, aff)
    first, last = out["levels"][0]["metric"][0], out["levels"][-1]["metric"][-1]
    print("inverted=%s: %.4f mm -> %.4f mm (ratio %.3f; the restatement: %.4f mm), mean cc %.4f -> %.4f"
          % (inverted, before, after, after / before, recorded(inverted)["error_after_mm"], first, last))
    assert [(L["shape"], L["iters"]) for L in out["levels"]] == [((10, 9, 8), 30), ((20, 18, 16), 15)]
    assert after <= wn.RECOVERY_RATIO * before and last > first
    assert abs(after - recorded(inverted)["error_after_mm"]) <= E2E_MARGIN_MM
    if not inverted:
        again = warp.register(fixed, aff, moving, aff, None, **wn.RECOVERY_OPTIONS)
        assert np.array_equal(again["disp"], out["disp"]) and again["levels"] == out["levels"]


def atlas_inputs(motor):
    fixed, moving, aff = wn.recovery_pair()
    rng = np.random.default_rng(8)
    res = {k: rng.random(gn.PHANTOM_SHAPE) for k in motor.STAT_QUANTITIES}
    res["TWC"] = fixed                                             # the reference volume the template is registered to
    res["fsol_4D"] = rng.random(gn.PHANTOM_SHAPE + (6,))
    res["T2s"] = np.logspace(1, np.log10(2000.0), 6)
    return res, aff, moving


def test_atlas_stats_filter_nonlinear(warp):
    motor = importlib.import_module(PKG + ".motor")
    res, aff, template = atlas_inputs(motor)
    lab, la, truth = wn.atlas_case()
    affine_only = motor.atlas_stats_filter(res, lab, la, aff, template=template, template_affine=aff)
    both = motor.atlas_stats_filter(res, lab, la, aff, template=template, template_affine=aff, nonlinear=True)
    wrong_affine = int((affine_only["labels_resampled"] != truth).sum())
    wrong_field = int((both["labels_resampled"] != truth).sum())
    print("labels that differ from the truth: %d affine only, %d with the field" % (wrong_affine, wrong_field))
    assert wrong_field < wrong_affine
    assert set(both) == set(affine_only) | {"disp", "warp_levels"} and np.array_equal(both["world"], affine_only["world"])
    assert both["disp"].shape == gn.PHANTOM_SHAPE + (3,) and [L["iters"] for L in both["warp_levels"]] == [30, 15]
    # a field estimated before is applied as it is
    given = motor.atlas_stats_filter(res, lab, la, aff, world=both["world"], disp=both["disp"])
    assert np.array_equal(given["labels_resampled"], both["labels_resampled"])
    with pytest.raises(ValueError, match="template"):
        motor.atlas_stats_filter(res, lab, la, aff, nonlinear=True)


def test_motor_atlas_stats_nonlinear_writes_the_field(warp, tmp_path):
    motor = importlib.import_module(PKG + ".motor")
    nifti = importlib.import_module(PKG + ".nifti")
    rs = importlib.import_module(PKG + ".resample")
    res, aff, template = atlas_inputs(motor)
    lab, la, truth = wn.atlas_case()
    out = str(tmp_path) + os.sep
    for k in motor.STAT_QUANTITIES + ("fsol_4D",):
        nifti.save(nifti.NiftiImage(res[k], aff), out + k + ".nii.gz")
    nifti.save(nifti.NiftiImage(lab, la), out + "atlas.nii.gz")
    nifti.save(nifti.NiftiImage(template, aff), out + "template.nii.gz")
    before = motor.motor_atlas_stats(out, out + "atlas.nii.gz", path_to_template=out + "template.nii.gz")
    files = set(os.listdir(out))
    assert not {"template_to_maps_warp.nii.gz", "template_warped.nii.gz"} & files
    got = motor.motor_atlas_stats(out, out + "atlas.nii.gz", path_to_template=out + "template.nii.gz", nonlinear={"iters": (0, 30, 15)})
    assert set(os.listdir(out)) == files | {"template_to_maps_warp.nii.gz", "template_warped.nii.gz"}
    field = nifti.load(out + "template_to_maps_warp.nii.gz")
    assert field.get_fdata().shape == gn.PHANTOM_SHAPE + (3,) and np.allclose(field.affine, aff) and np.array_equal(field.get_fdata(), got["disp"])
    A = rs.voxel_matrix(aff, nifti.load(out + "template.nii.gz").affine, got["world"])
    warped = nifti.load(out + "template_warped.nii.gz").get_fdata()
    assert np.allclose(warped, np.asarray(wn.warp(nifti.load(out + "template.nii.gz").get_fdata(), A, got["disp"], 1, 0.0, np.float64), dtype=np.float64), atol=1e-5)
    assert np.array_equal(nifti.load(out + "ROIs_resampled.nii.gz").get_fdata(), got["labels_resampled"])
    assert int((got["labels_resampled"] != truth).sum()) < int((before["labels_resampled"] != truth).sum())
    assert np.array_equal(got["world"], before["world"])
