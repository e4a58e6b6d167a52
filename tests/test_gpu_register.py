"""The registration cost on the device (met2_register_index, met2_register_cost; include/met2_hip.h states the contract) against its numpy
restatement in long double (tests/tools/register_numpy.py, which tests/test_register_host.py holds against scipy), and the registration end
to end with device costs.
Cost.  n_inside equal; |cost - long-double cost| within BOUND = 16 x the largest such difference measured on an MI355X over these very cases
(profiles/register_parity.json: head-room for another rounding order on another device), which may not exceed 1e-10 -- far below any ftol the
search can use; a larger error would be a defect, not rounding.  With MET2_REGISTER_PARITY_OUT=<file> the module writes what it measured there.
Grids: fixed 9 x 7 x 5 (315 voxels: no multiple of a wave or a run), 17 x 16 x 33 (8 976 = 35 runs and 16 voxels) and 16 x 16 x 1, the last
with a moving volume that has an axis of 1 too; 1, 2, 64 and 256 bins; 1, 3, 17 and 256 (the maximum) candidates; a tenth of the voxels excluded
(-1).  Among the candidates: one that puts the last fixed sample exactly on the last moving sample of every axis, one wholly outside, shifts
that leave every share of the voxels inside.  Bins that hold 0, 1, 255, 256 and 257 voxels (a run is 256), a constant moving volume, a pair
of candidates just under and just over min_overlap, the same bits from call to call and wherever a candidate stands, the refusals.
End to end: register and atlas_stats_filter(template=...) on the 20 x 18 x 16 phantom within twice what the restatement-driven search on
the CPU reaches (profiles/register_recovery.json), one fixed voxel at the most; motor_atlas_stats(path_to_template=...) on files."""
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

pytestmark = pytest.mark.gpu

PKG = "multicomponent-t2-toolbox_amd"
CEILING = 1e-10
MEASURED = {"max_abs_cost_error": 0.0, "per_kind": {k: 0.0 for k in gn.KINDS}, "n_costs": 0}
GRIDS = {"small": ((9, 7, 5), (11, 9, 6)), "long": ((17, 16, 33), (15, 18, 30)), "flat": ((16, 16, 1), (12, 10, 1))}
MAX_K = 256


def _json(name):
    path = os.path.join(ROOT, "profiles", name)
    assert os.path.exists(path), "%s is missing: it holds the measured figures the bounds derive from" % path
    return json.load(open(path))


def bound():
    b = 16.0 * float(_json("register_parity.json")["max_abs_cost_error"])
    assert 0.0 < b <= CEILING, "the measured cost error puts the bound at %g: above %g it is a defect, not rounding" % (b, CEILING)
    return b


@pytest.fixture(scope="module")
def reg():
    yield importlib.import_module(PKG + ".register")
    path = os.environ.get("MET2_REGISTER_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(MEASURED, reference="tests/tools/register_numpy.py in long double", bound_factor=16, ceiling=CEILING,
                           device=torch.cuda.get_device_name(0)), f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def motor():
    return importlib.import_module(PKG + ".motor")


def candidates(fdims, mdims):
    """256 transforms of a grid pair, the edge cases first: [0] the last fixed sample on the last moving sample of every axis (identity plus
    the difference of the axes), [1] wholly outside, [2] the identity, then shifts, scalings and rotations about the centres"""
    rng = np.random.default_rng(list(fdims) + list(mdims))
    cf, cm = (np.array(fdims) - 1.0) / 2.0, (np.array(mdims) - 1.0) / 2.0
    out = [np.column_stack([np.eye(3), np.array(mdims, dtype=np.float64) - np.array(fdims)]),
           np.column_stack([np.eye(3), [-1000.0, 0.0, 0.0]]), np.column_stack([np.eye(3), np.zeros(3)])]
    while len(out) < MAX_K:
        ang = np.deg2rad(rng.uniform(-25.0, 25.0, 3))
        shift = rng.uniform(-0.35, 0.35, 3) * np.array(mdims)
        if mdims[2] == 1:                                          # a single slice: only what keeps c_z = 0 exactly can be inside
            ang[0] = ang[1] = shift[2] = 0.0
        R = np.eye(3)
        for a, (i, j) in zip(ang, ((1, 2), (0, 2), (0, 1))):
            G = np.eye(3)
            G[i, i] = G[j, j] = np.cos(a)
            G[i, j], G[j, i] = -np.sin(a), np.sin(a)
            R = R @ G
        M = R @ np.diag(rng.uniform(0.7, 1.3, 3) * (np.maximum(np.array(mdims) - 1.0, 0.0) / np.maximum(np.array(fdims) - 1.0, 1.0)))
        if len(out) % 4 == 0:
            M = np.eye(3)                                          # pure shifts by fractions of a voxel
        out.append(np.column_stack([M, cm - M @ cf + shift]))
    return np.ascontiguousarray(np.stack(out))


_CASE = {}


def case(grid):
    """the inputs of a grid pair and the restatement's samples, computed once: fixed, moving, excluded, A [256, 3, 4], [(y, inside)] per candidate"""
    if grid not in _CASE:
        fdims, mdims = GRIDS[grid]
        rng = np.random.default_rng(sum(fdims) + 7)
        fixed = rng.random(fdims)
        moving = rn.volume(rng, mdims, 1, vmax=1.5)[0] + 0.25
        excluded = rng.random(fdims) < 0.1
        A = candidates(fdims, mdims)
        _CASE[grid] = (fixed, moving, excluded, A, [gn.sample(moving, a, fdims) for a in A])
    return _CASE[grid]


def bins_of(fixed, excluded, n_bins):
    b = np.minimum(np.floor(fixed * n_bins), n_bins - 1).astype(np.int32)
    b[excluded] = -1
    return b


def check(reg, fixed, bins, moving, A, samples, n_bins, min_overlap, kinds=gn.KINDS):
    """the device against the restatement for the candidates A; -> {kind: (n_inside, cost)} of the device"""
    got = {}
    worst_err = 0.0
    for kind in kinds:
        n, c = reg.prepare(fixed, bins, moving, kind, n_bins, min_overlap)(A)
        want = [gn.cost_of_sample(fixed, bins, moving, y, ins, kind, n_bins, min_overlap) for y, ins in samples]
        assert n.dtype == np.int64 and np.array_equal(n, [w[0] for w in want]), kind
        assert np.isfinite(c).all(), kind
        wc = np.array([w[1] for w in want])
        is_worst = wc == gn.worst(kind)
        assert np.array_equal(c[is_worst], wc[is_worst]), kind      # the worst value exactly
        err = float(np.abs(c - wc)[~is_worst].max()) if (~is_worst).any() else 0.0
        MEASURED["per_kind"][kind] = max(MEASURED["per_kind"][kind], err)
        MEASURED["max_abs_cost_error"] = max(MEASURED["max_abs_cost_error"], err)
        MEASURED["n_costs"] += len(wc)
        worst_err = max(worst_err, err)
        got[kind] = (n, c)
    print("max |cost - long double| = %.3g" % worst_err)
    assert worst_err <= bound()
    return got


SWEEP = [("small", b, k) for b in (1, 2, 64, 256) for k in (1, 3, 17, MAX_K)] + [("long", b, k) for b, k in ((1, 17), (2, 3), (64, 17), (256, 3))] + \
        [("flat", b, k) for b, k in ((2, 1), (64, 17), (1, 3))]


@pytest.mark.parametrize("grid,n_bins,K", SWEEP)
def test_cost_against_restatement(reg, grid, n_bins, K):
    fixed, moving, excluded, A, samples = case(grid)
    got = check(reg, fixed, bins_of(fixed, excluded, n_bins), moving, A[:K], samples[:K], n_bins, 0.25)
    n = got["corratio"][0]
    incl = int((~excluded).sum())
    assert n[0] > 0 and (K < 2 or n[1] == 0)                       # the last-sample candidate is inside on a whole corner block; [1] is outside
    if K >= 17:                                                    # the shares of voxels inside spread from none to most
        assert n.max() > 0.75 * incl and (n == 0).sum() >= 1 and 0 < np.median(n) < n.max()


def test_last_sample_is_inside(reg):
    """candidate 0 puts fixed voxel (mx - 1, my - 1, mz - 1) exactly on the last moving sample of every axis: it counts, its taps beyond are mirrored"""
    fixed, moving, excluded, A, samples = case("small")
    y, ins = samples[0]
    assert ins.all() and np.array_equal(rn.coords(A[0], fixed.shape)[:, -1, -1, -1], np.array(moving.shape) - 1.0)
    bins = bins_of(fixed, np.zeros_like(excluded), 4)
    got = check(reg, fixed, bins, moving, A[:1], samples[:1], 4, 1.0)      # min_overlap = 1: every voxel must be inside, and is
    assert got["corratio"][0][0] == fixed.size and got["leastsq"][1][0] < 1e3


def test_run_length_bins(reg):
    """bins of 0, 1, 255, 256 and 257 voxels (a run is 256), the rest in three more; excluded voxels in between"""
    fixed, moving, excluded, A, samples = case("long")
    assert reg.limits()["run"] == 256
    order = np.random.default_rng(11).permutation(fixed.size)
    bins = np.full(fixed.size, -1, dtype=np.int32)
    at = 0
    for b, count in ((1, 1), (2, 255), (3, 256), (4, 257), (5, 3000), (6, 1), (7, 2500)):     # bin 0 stays empty; 2 706 voxels stay excluded
        bins[order[at:at + count]] = b
        at += count
    bins = bins.reshape(fixed.shape)
    assert np.array_equal(np.bincount(bins[bins >= 0], minlength=8), [0, 1, 255, 256, 257, 3000, 1, 2500])
    check(reg, fixed, bins, moving, A[:17], samples[:17], 8, 0.25)
    one = np.where(bins == 4, 0, -1).astype(np.int32)              # one bin of 257 alone: two runs, the second of one voxel
    check(reg, fixed, one, moving, A[:3], samples[:3], 1, 0.0)


def test_min_overlap_and_outside(reg):
    """two shifts along x that leave 4 and 5 of the 9 planes inside; min_overlap between their shares: the one under it takes the worst value
    exactly, the one over it does not; so does the candidate that is wholly outside, whatever min_overlap"""
    fixed, moving, excluded, _, _ = case("small")
    A = np.stack([np.column_stack([np.eye(3), [7.0, 0.5, 0.25]]), np.column_stack([np.eye(3), [6.0, 0.5, 0.25]]), np.column_stack([np.eye(3), [0.0, 0.0, 50.0]])])
    samples = [gn.sample(moving, a, fixed.shape) for a in A]
    bins = bins_of(fixed, excluded, 16)
    incl = bins >= 0
    n_under, n_over = int((incl & samples[0][1]).sum()), int((incl & samples[1][1]).sum())
    assert samples[0][1][:4].all() and not samples[0][1][4:].any() and samples[1][1][:5].all() and n_under < n_over
    min_overlap = 0.5 * (n_under + n_over) / incl.sum()
    got = check(reg, fixed, bins, moving, A, samples, 16, min_overlap)
    for kind in gn.KINDS:
        n, c = got[kind]
        assert list(n) == [n_under, n_over, 0] and c[0] == gn.worst(kind) and c[2] == gn.worst(kind) and c[1] < gn.worst(kind)
    # exactly at the threshold a candidate counts (n_inside < min_overlap n_included is false): 4 planes inside of 8 included, min_overlap 1 / 2
    eight = np.zeros(fixed.shape, dtype=np.int32)
    eight[8] = -1
    exact = check(reg, fixed, eight, moving, A[:1], samples[:1], 1, 0.5, kinds=("leastsq",))
    assert exact["leastsq"][0][0] == 4 * 35 and exact["leastsq"][1][0] < gn.worst("leastsq")
    got0 = check(reg, fixed, bins, moving, A, samples, 16, 0.0)      # min_overlap = 0: only the empty candidate is refused
    assert got0["corratio"][1][0] < 1.0 and got0["corratio"][1][2] == 1.0


def test_constant_volumes(reg):
    """zero variance where a ratio needs one: the worst value exactly, never NaN; leastsq has no ratio and stays a mean"""
    fixed, moving, excluded, A, samples = case("small")
    bins = bins_of(fixed, excluded, 8)
    flat = np.full(moving.shape, 3.7)
    flat_samples = [gn.sample(flat, a, fixed.shape) for a in A[:17]]
    got = check(reg, fixed, bins, flat, A[:17], flat_samples, 8, 0.0)
    assert (got["corratio"][1] == 1.0).all() and (got["normcorr"][1] == 1.0).all()
    inside = got["leastsq"][0] > 0
    assert (got["leastsq"][1][inside] < 20.0).all() and (got["leastsq"][1][~inside] == gn.LEASTSQ_WORST).all()
    got = check(reg, np.full(fixed.shape, -2.5), bins, moving, A[:17], samples[:17], 8, 0.0, kinds=("normcorr",))
    assert (got["normcorr"][1] == 1.0).all()
    zero = check(reg, fixed, bins, np.zeros(moving.shape), A[:3], [gn.sample(np.zeros(moving.shape), a, fixed.shape) for a in A[:3]], 8, 0.0)
    assert (zero["corratio"][1] == 1.0).all()


@pytest.mark.parametrize("kind", gn.KINDS)
def test_same_bits_wherever_a_candidate_stands(reg, kind):
    fixed, moving, excluded, A, _ = case("long")
    f = reg.prepare(fixed, bins_of(fixed, excluded, 64), moving, kind, 64, 0.25)
    n17, c17 = f(A[:17])
    again = f(A[:17])
    assert np.array_equal(again[0], n17) and np.array_equal(again[1].view(np.int64), c17.view(np.int64))
    for k in (0, 5, 16):
        n1, c1 = f(A[k:k + 1])
        assert n1[0] == n17[k] and c1.view(np.int64)[0] == c17.view(np.int64)[k]
    perm = np.roll(np.arange(17), 6)                               # every candidate at another place of the batch
    n_p, c_p = f(A[perm])
    assert np.array_equal(n_p, n17[perm]) and np.array_equal(c_p.view(np.int64), c17[perm].view(np.int64))
    n_all, c_all = f(A)                                            # and inside the largest batch
    assert np.array_equal(n_all[:17], n17) and np.array_equal(c_all[:17].view(np.int64), c17.view(np.int64))
    g = reg.prepare(fixed, bins_of(fixed, excluded, 64), moving, kind, 64, 0.25)       # a fresh index
    assert np.array_equal(g(A[:17])[1].view(np.int64), c17.view(np.int64))


def test_tensors_and_the_stage_wrapper(reg):
    fixed, moving, excluded, A, samples = case("small")
    bins = bins_of(fixed, excluded, 8)
    n, c = reg.prepare(fixed, bins, moving, "corratio", 8, 0.25)(A[:5])
    tn, tc = reg.prepare(torch.as_tensor(fixed, device="cuda"), torch.as_tensor(bins, device="cuda"), torch.as_tensor(moving, device="cuda"), "corratio", 8, 0.25)(A[:5])
    assert tn.is_cuda and tc.is_cuda and np.array_equal(tn.cpu().numpy(), n) and np.array_equal(tc.cpu().numpy(), c)
    # cost(): the module's intensity rule, then the same entry
    mask = ~excluded
    fs = reg.scale_intensity(fixed, mask)
    for kind, nb in (("corratio", 8), ("normcorr", 1)):           # n_bins counts for corratio; the other two index every voxel in one bin
        want = reg.prepare(fs, reg.bin_intensity(fs, nb, fixed, mask), reg.scale_intensity(moving), kind, nb, 0.1)(A[:5])
        got = reg.cost(fixed, moving, A[:5], kind, 8, mask, 0.1)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match="finite"):
        reg.prepare(np.where(excluded, np.nan, fixed), bins, moving)


def test_refusals_leave_the_outputs_untouched(reg):
    _lib = importlib.import_module(PKG + "._lib")
    L = _lib.lib()
    fdims, mdims = GRIDS["small"]
    fixed, moving, excluded, A, _ = case("small")
    i3 = lambda d: (C.c_int32 * 3)(*d)
    r2 = (C.c_double * 2)(0.0, 2.0)
    dev = torch.device("cuda", 0)
    f, m = torch.as_tensor(fixed, device=dev), torch.as_tensor(moving, device=dev)
    b = torch.as_tensor(bins_of(fixed, excluded, 8), device=dev)
    ib, wb = reg.work_bytes(fdims, 8, 3)
    index = torch.full((ib // 4,), -77, dtype=torch.int32, device=dev)
    work = torch.zeros(wb // 8 + 1, dtype=torch.float64, device=dev)
    n_out = torch.full((3,), -5, dtype=torch.int64, device=dev)
    c_out = torch.full((3,), -5.0, dtype=torch.float64, device=dev)
    a = np.ascontiguousarray(A[:3])
    bad = a.copy()
    bad[1, 0, 0] = np.inf

    def cost(kind=0, bins=8, K=3, mat=a, mo=0.25, nbytes=wb, md=mdims):
        return L.met2_register_cost(0, kind, i3(fdims), bins, index.data_ptr(), f.data_ptr(), r2, i3(md), m.data_ptr(), r2, K, mat.ctypes.data_as(_lib._dp), mo,
                                    work.data_ptr(), nbytes, n_out.data_ptr(), c_out.data_ptr(), None)

    assert L.met2_register_index(0, i3(fdims), b.data_ptr(), 8, index.data_ptr(), ib - 4, None) == -1
    assert L.met2_register_index(0, i3(fdims), b.data_ptr(), 257, index.data_ptr(), ib, None) == -2
    torch.cuda.synchronize()
    assert bool((index == -77).all())
    for rc, kw in ((-1, {"kind": 5}), (-1, {"bins": 0}), (-2, {"K": 257}), (-1, {"mat": bad}), (-1, {"mo": 2.0}), (-1, {"nbytes": wb - 8}), (-2, {"md": (11, 9, 600)})):
        assert cost(**kw) == rc, kw
    torch.cuda.synchronize()
    assert bool((n_out == -5).all()) and bool((c_out == -5.0).all()) and bool((work == 0).all())
    assert L.met2_register_index(0, i3(fdims), b.data_ptr(), 8, index.data_ptr(), ib, None) == 0 and cost() == 0
    torch.cuda.synchronize()
    want = reg.prepare(fixed, bins_of(fixed, excluded, 8), moving, "corratio", 8, 0.25)(a)
    assert np.array_equal(n_out.cpu().numpy(), want[0]) and bool((c_out >= 0).all())


# ---------------------------------------------------------------- end to end, on the phantom of the host test

def recovery(name):
    row = _json("register_recovery.json")["cases"][name]
    assert row["mean_displacement_mm"] < 0.5 * gn.CAP_MM             # the restatement itself stays well inside the cap
    return min(2.0 * row["mean_displacement_mm"], gn.CAP_MM), 2.0 * row["label_share"]


@pytest.mark.parametrize("name", ["rigid6", "affine12"])
def test_register_recovers_the_transform(reg, motor, name):
    true_world, dof, kind, (fx, fa, mv, ma, mask) = gn.e2e_case(name, reg)
    out = reg.register(fx, fa, mv, ma, dof=dof, cost=kind)
    got = gn.mean_displacement(out["world"], true_world, mask, fa)
    limit, _ = recovery(name)
    print("%s: mean displacement %.4f mm (bound %.4f), cost %.5f, %d evaluations in %d launches" %
          (name, got, limit, out["cost"], sum(l["n_eval"] for l in out["levels"]), sum(l["n_calls"] for l in out["levels"])))
    assert got <= limit
    if name == "rigid6":
        assert np.array_equal(motor.register_filter(fx, fa, mv, ma, dof=dof, cost=kind), out["world"])      # the driver's face; deterministic


def atlas_inputs(motor, reg):
    true_world, dof, kind, (fx, fa, mv, ma, mask) = gn.e2e_case("rigid6", reg)
    rng = np.random.default_rng(8)
    res = {k: rng.random(gn.PHANTOM_SHAPE) for k in motor.STAT_QUANTITIES}
    res["TWC"] = fx                                                # the reference volume the template is registered to
    res["fsol_4D"] = rng.random(gn.PHANTOM_SHAPE + (6,))
    res["T2s"] = np.logspace(1, np.log10(2000.0), 6)
    return true_world, res, fa, mv, ma


def test_atlas_stats_filter_with_a_template(reg, motor):
    true_world, res, fa, template, ta = atlas_inputs(motor, reg)
    labels = gn.atlas_labels()
    want = motor.atlas_stats_filter(res, labels, ta, fa, world=true_world)
    got = motor.atlas_stats_filter(res, labels, ta, fa, template=template)
    share = float((got["labels_resampled"] != want["labels_resampled"]).mean())
    _, limit = recovery("rigid6")
    print("share of voxels with another label: %.5f (bound %.5f)" % (share, limit))
    assert share <= limit
    assert set(got) == set(want) | {"world"} and list(got["labels"]) == [1, 2, 3, 7] and (want["labels_resampled"] > 0).sum() > 400
    assert np.array_equal(got["world"], motor.register_filter(res["TWC"], fa, template, ta))
    with pytest.raises(ValueError, match="not both"):
        motor.atlas_stats_filter(res, labels, ta, fa, world=true_world, template=template)


def test_motor_atlas_stats_with_and_without_a_template(reg, motor, tmp_path):
    nifti = importlib.import_module(PKG + ".nifti")
    rs = importlib.import_module(PKG + ".resample")
    true_world, res, fa, template, ta = atlas_inputs(motor, reg)
    out = str(tmp_path) + os.sep
    for k in motor.STAT_QUANTITIES + ("fsol_4D",):
        nifti.save(nifti.NiftiImage(res[k], fa), out + k + ".nii.gz")
    labels = gn.atlas_labels()
    nifti.save(nifti.NiftiImage(labels, ta), out + "atlas.nii.gz")
    nifti.save(nifti.NiftiImage(template, ta), out + "template.nii.gz")
    np.savetxt(out + "world.txt", true_world)
    # without the new keywords: what it gave before -- label_stats_filter on the labels the given matrix resamples, the same keys, no new file
    st = motor.motor_atlas_stats(out, out + "atlas.nii.gz", out + "world.txt", names={1: "CC"})
    back = {k: nifti.load(out + k + ".nii.gz").get_fdata() for k in motor.STAT_QUANTITIES + ("fsol_4D",)}
    back["T2s"] = res["T2s"]
    A = rs.voxel_matrix(nifti.load(out + "MWF.nii.gz").affine, nifti.load(out + "atlas.nii.gz").affine, true_world)
    want_lab = rn.resample_labels(labels, A, gn.PHANTOM_SHAPE)
    want = motor.label_stats_filter(back, want_lab)
    assert np.array_equal(st["labels_resampled"], want_lab) and set(st) == set(want) | {"labels_resampled", "all"}
    for k in motor.STAT_KEYS:
        assert np.array_equal(st[k], want[k], equal_nan=True), k
    assert sorted(os.listdir(out)) == sorted([k + ".nii.gz" for k in motor.STAT_QUANTITIES + ("fsol_4D",)] +
                                             ["atlas.nii.gz", "template.nii.gz", "world.txt", "ROIs_resampled.nii.gz", "table_roi_stats.csv", "table_roi_spectra.csv"])
    # with a template: the matrix is estimated against TWC.nii.gz (there is no Data_avg.nii.gz), written in both conventions, and used
    got = motor.motor_atlas_stats(out, out + "atlas.nii.gz", path_to_template=out + "template.nii.gz", names={1: "CC"})
    world = np.loadtxt(out + "template_to_maps_world.txt")
    assert np.array_equal(world, got["world"])
    limit, share_limit = recovery("rigid6")
    mask = res["TWC"] > 0.05
    assert gn.mean_displacement(world, true_world, mask, fa) <= limit
    assert float((got["labels_resampled"] != st["labels_resampled"]).mean()) <= share_limit
    maps_aff, tpl_aff = nifti.load(out + "TWC.nii.gz").affine, nifti.load(out + "template.nii.gz").affine
    assert np.allclose(rs.from_flirt(np.loadtxt(out + "template_to_maps_flirt.mat"), tpl_aff, template.shape, maps_aff, gn.PHANTOM_SHAPE), world, atol=1e-9)
    on_maps = nifti.load(out + "template_resampled.nii.gz")
    assert on_maps.get_fdata().shape == gn.PHANTOM_SHAPE and np.allclose(on_maps.affine, maps_aff)
    assert np.allclose(on_maps.get_fdata(), rn.resample(nifti.load(out + "template.nii.gz").get_fdata(), rs.voxel_matrix(maps_aff, tpl_aff, world), gn.PHANTOM_SHAPE),
                       atol=1e-5)
    # Data_avg.nii.gz, where present, is the reference: a copy of the phantom gives the same matrix
    nifti.save(nifti.NiftiImage(res["TWC"], fa), out + "Data_avg.nii.gz")
    assert np.array_equal(motor.motor_atlas_stats(out, out + "atlas.nii.gz", path_to_template=out + "template.nii.gz")["world"], got["world"])
