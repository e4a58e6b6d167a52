"""The non-linear registration of warp.py on the CPU: the loop is warp.register's own, its five stages and the pyramid's filters are the
numpy restatement (tests/tools/warp_numpy.py in fp64, register_numpy.FILTERS), so no device is needed.
Recovery.  Fixed: register_numpy's phantom on its 20 x 18 x 16 grid at 2 mm.  Moving: the phantom evaluated analytically at P + d(P) on the
same grid, d = 3 (sin(y/9 + 0.3) cos(z/11), sin(z/8 - 0.5) cos(x/10), sin(x/7 + 1) cos(y/12)) mm; once in the same contrast, once as
0.9 - 0.8 v + 0.3 v^2.  The error of a voxel is |u 2 mm + d(P + u 2 mm)|, averaged over fixed > 0.05: 2.80 mm before.  Required: at most 0.65
of that after, and the last metric above the first.  (Measured with this restatement: 1.23 mm = 0.44 in the same contrast, 1.38 mm = 0.49
inverted; profiles/warp_recovery.json.  What is left is the homogeneous interior, which no intensity metric sees.)
The rim.  register scales both images to [0, 1] (register.scale_intensity), which takes a constant offset out again; a background that is
not zero AFTER the scaling is what shows the false edge at the rim of the field of view, and the inverted contrast has the brightest one.
With the moving image inverted and offset by +0.2 the metric rises on every level; with the plain clamped gradient in place of the rule's
(neighbours in the grid AND inside) it falls on the fine level -- so the case tells the two apart."""
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import register_numpy as gn                                        # noqa: E402
import resample_numpy as rn                                        # noqa: E402
import warp_numpy as wn                                            # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"


@pytest.fixture(scope="module")
def warp():
    return importlib.import_module(PKG + ".warp")


def run(warp, inverted, offset=0.0, plain=False, **over):
    fixed, moving, aff = wn.recovery_pair(inverted, offset)
    out = warp.register(fixed, aff, moving, aff, None, stages=wn.stages(np.float64, plain), filters=gn.FILTERS, **dict(wn.RECOVERY_OPTIONS, **over))
    return out, fixed, aff


@pytest.fixture(scope="module")
def recovered(warp):
    return {inv: run(warp, inv) for inv in (False, True)}


@pytest.mark.parametrize("inverted", (False, True))
def test_recovers_a_smooth_field(recovered, inverted):
    out, fixed, aff = recovered[inverted]
    before = wn.recovery_error(np.zeros(fixed.shape + (3,)), fixed, aff)
    after = wn.recovery_error(out["disp"], fixed, aff)
    first, last = out["levels"][0]["metric"][0], out["levels"][-1]["metric"][-1]
    print("inverted=%s: %.3f mm -> %.3f mm (ratio %.3f), mean cc %.4f -> %.4f" % (inverted, before, after, after / before, first, last))
    assert [(L["shape"], L["iters"], len(L["metric"])) for L in out["levels"]] == [((10, 9, 8), 30, 30), ((20, 18, 16), 15, 15)]   # 5 x 5 x 4 is skipped
    assert out["disp"].shape == fixed.shape + (3,) and out["disp"].dtype == np.float64 and np.array_equal(out["world"], np.eye(4))
    assert 2.7 < before < 2.9
    assert after <= wn.RECOVERY_RATIO * before
    assert last > first


def test_metric_rises_with_a_bright_background_and_the_plain_gradient_fails(warp):
    out, _, _ = run(warp, True, 0.2)
    for L in out["levels"]:
        assert L["metric"][-1] > L["metric"][0], L
    plain, _, _ = run(warp, True, 0.2, plain=True)
    fine = plain["levels"][-1]["metric"]
    assert fine[-1] < fine[0], "the plain clamped gradient no longer fails here: the case does not test the rule"
    # a constant offset alone is taken out by the intensity scaling: the same field as without it, to rounding
    off, _, _ = run(warp, False, 0.2)
    assert off["levels"][-1]["metric"][-1] > off["levels"][0]["metric"][0]


def test_two_runs_give_the_same_bits(warp, recovered):
    again, _, _ = run(warp, False)
    assert np.array_equal(again["disp"], recovered[False][0]["disp"])
    assert again["levels"] == recovered[False][0]["levels"]


def test_zero_iterations_return_a_zero_field(warp):
    out, fixed, _ = run(warp, False, iters=(0, 0, 0))
    assert out["disp"].shape == fixed.shape + (3,) and not out["disp"].any()
    assert [(L["iters"], L["metric"]) for L in out["levels"]] == [(0, []), (0, [])]
    one, _, _ = run(warp, False, iters=0, scales_mm=[2.0])
    assert not one["disp"].any() and len(one["levels"]) == 1


def test_a_level_change_keeps_the_field_in_millimetres(warp):
    # all iterations on the coarse level: the field of the fixed grid is the coarse one carried over, twice the voxels, the same millimetres
    out, fixed, aff = run(warp, False, iters=(0, 30, 0))
    coarse, _, _ = run(warp, False, iters=(0, 30), scales_mm=[8.0, 4.0])
    assert coarse["disp"].shape == fixed.shape + (3,)
    assert np.array_equal(out["disp"], coarse["disp"])
    assert 0.3 < np.abs(out["disp"]).max() < 3.0


def test_refusals(warp):
    fixed, moving, aff = wn.recovery_pair()
    ok = dict(stages=wn.STAGES, filters=gn.FILTERS)
    for bad, match in ((dict(radius=0), "radius"), (dict(radius=5), "radius"), (dict(radius=2.5), "radius"), (dict(step=0.0), "step"),
                       (dict(step=float("nan")), "step"), (dict(sigma_fluid=-1.0), "sigma"), (dict(sigma_elastic=float("inf")), "sigma"),
                       (dict(sigma_fluid=9.0), "sigma"), (dict(iters=(30, 30)), "iters"), (dict(iters=(30, -1, 15)), "iters"),
                       (dict(iters=(1.5, 1, 1)), "iters"), (dict(scales_mm=[]), "scales_mm"), (dict(scales_mm=[-1.0], iters=(1,)), "scale"),
                       (dict(filters=None), "filters"), (dict(stages={"warp": wn.STAGES["warp"]}), "stages")):
        with pytest.raises(ValueError, match=match):
            warp.register(fixed, aff, moving, aff, None, **dict(ok, **bad))
    with pytest.raises(ValueError, match="world"):
        warp.register(fixed, aff, moving, aff, np.zeros((4, 4)), **ok)
    with pytest.raises(ValueError, match="three axes"):
        warp.register(fixed[0], aff, moving, aff, None, **ok)


def test_labels_through_the_field_are_closer_to_the_truth(recovered):
    # what atlas_stats_filter(nonlinear=True) does with the labels, on the CPU (the filter itself takes its statistics on the device:
    # tests/test_gpu_warp.py runs it): the atlas labels through the estimated field against the labels through the matrix alone
    out, fixed, aff = recovered[False]
    lab, la, truth = wn.atlas_case()
    A = (np.linalg.inv(la) @ aff)[:3]
    affine_only = rn.resample_labels(lab, A, fixed.shape)
    through_field = wn.warp_labels(lab, A, out["disp"])
    wrong_affine, wrong_field = int((affine_only != truth).sum()), int((through_field != truth).sum())
    print("labels that differ from the truth: %d with the matrix alone, %d through the field (of %d labelled)" % (wrong_affine, wrong_field, (truth > 0).sum()))
    assert (truth > 0).sum() > 400 and wrong_affine > 100
    assert wrong_field < wrong_affine


def test_filters_refuse_nonlinear_without_a_template():
    filters = importlib.import_module(PKG + ".filters")
    res = {"MWF": np.zeros((2, 2, 2)), "TWC": np.zeros((2, 2, 2))}
    with pytest.raises(ValueError, match="template"):
        filters.atlas_stats_filter(res, np.zeros((2, 2, 2), dtype=np.int32), np.eye(4), np.eye(4), nonlinear=True)
    with pytest.raises(ValueError, match="nonlinear must be"):
        filters.atlas_stats_filter(res, np.zeros((2, 2, 2), dtype=np.int32), np.eye(4), np.eye(4), template=np.zeros((2, 2, 2)), nonlinear=1)
    motor = importlib.import_module(PKG + ".motor")
    with pytest.raises(ValueError, match="path_to_template"):
        motor.motor_atlas_stats("nowhere/", "nowhere/atlas.nii.gz", nonlinear=True)
    for name in ("warp_register_filter", "warp_filter", "warp_labels_filter"):
        assert getattr(motor, name) is getattr(filters, name)


def test_the_cases_of_the_device_tests_are_what_they_claim():
    # no device: the properties tests/test_gpu_warp.py asserts of its inputs, and the records its bounds come from
    import json
    for grid in wn.GRIDS:
        src = wn.source_dims(grid)
        _, ins, c = wn.warp(wn.case_volume(grid, 1), wn.case_transform(grid), wn.case_field(grid), 1, 0.0, np.float64, return_inside=True, return_coords=True)
        assert wn.coordinate_margin(c, src) > wn.MARGIN and ins.any(), grid
        F, W, m = wn.lncc_inputs(grid)
        for r in wn.RADII:
            sums = np.asarray(wn.lncc_sums(F, W, m, r, np.float64))
            _, _, valid, (B, C) = wn.lncc_force(F, W, m, sums, wn.FORCE_EPS, np.longdouble, return_terms=True)
            assert wn.eps_margin(B, C, m, sums[0], wn.FORCE_EPS), (grid, r)
            assert valid.any() or min(grid) == 1, (grid, r)
    rec = json.load(open(os.path.join(ROOT, "profiles", "warp_recovery.json")))
    for key, inverted in (("same_contrast", False), ("inverted", True)):
        assert rec[key]["ratio"] <= rec["required_ratio"] == wn.RECOVERY_RATIO
        assert rec[key + "_plain_gradient"]["error_after_mm"] > 0.0
    assert rec["inverted_plain_gradient"]["ratio"] > wn.RECOVERY_RATIO        # the record of why the rule looks at `inside`
    par = json.load(open(os.path.join(ROOT, "profiles", "warp_parity.json")))
    assert all(0.0 < 16.0 * v <= par["ceiling"] == 1e-12 for v in par["max_rel_error"].values())


def test_the_recorded_recovery_is_the_restatement_s(recovered):
    import json
    rec = json.load(open(os.path.join(ROOT, "profiles", "warp_recovery.json")))
    for key, inverted in (("same_contrast", False), ("inverted", True)):
        out, fixed, aff = recovered[inverted]
        assert abs(wn.recovery_error(out["disp"], fixed, aff) - rec[key]["error_after_mm"]) < 1e-6
