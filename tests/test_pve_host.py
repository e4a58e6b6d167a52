"""Host tests (no GPU) of the partial-volume maps: the numpy restatement of include/met2_hip.h's met2_partial_volume (tests/tools/pve_numpy.py)
does what a mixel model must, no type of the inputs tests/test_gpu_pve.py runs hangs on a rounding (the long-double restatement's smallest
relative energy gap over all visits is far above 1e-9, and fp64 gives the same types: that is what lets the GPU test ask for equal types),
the fractions it gives on a phantom with known fractions beat the hard labels, and the drivers take segment='pve' and refuse a bad
`segment` before any device work."""
import importlib
import inspect
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import pve_numpy as pn                                             # noqa: E402
import seg_numpy as sn                                             # noqa: E402

PKG = "multicomponent-t2-toolbox_amd"


def staged(name="tile+1", dtype=np.float64):
    c = pn.case(name)
    return c, pn.partial_volume(c["v"], c["seg"], c["prob"], c["voxel"], dtype=dtype)


def test_beta_pv_zero_is_the_plain_argmin():
    c, r = staged()
    E, om, live = r["E"], r["om"], r["live"]
    assert live.all() and np.array_equal(r["types0"][om], np.argmin(E[:, om], axis=0))
    assert len(np.unique(r["types0"][om])) == 5                         # pure and mixed types are all in use
    assert np.array_equal(pn.icm(r["types0"], E, live, r["w"], 0.0, 3), r["types0"])
    assert not np.array_equal(r["mixeltype"], r["types0"])               # the prior does change types


def test_a_sweep_never_raises_the_total_energy():
    c, r = staged("aniso")
    El, wl = r["E"].astype(np.longdouble), r["w"].astype(np.longdouble)
    for beta_pv in (0.3, 2.0):
        trace = []
        pn.icm(r["types0"], r["E"], r["live"], r["w"], beta_pv, 8, trace)
        U = [pn.total_energy(t, El, wl, np.longdouble(beta_pv)) for t in [r["types0"]] + trace]
        scale = abs(U[0])
        for before, after in zip(U[:-1], U[1:]):                         # per colour pass; 1e-15: the rounding of fp64 energies that tie
            assert after <= before + 1e-15 * scale, beta_pv
        assert U[-1] < U[0]
        assert np.array_equal(trace[-1], trace[-2])                      # 8 sweeps converge here


def test_the_distance_of_types():
    for K in (1, 2, 3, 8):
        d = pn.delta2_table(K)
        assert d.shape == (2 * K - 1, 2 * K - 1) and np.array_equal(d, d.T) and np.all(np.diag(d) == 0)
        assert set(np.unique(d)) <= {0, 1, 2}
    d = pn.delta2_table(3)                                              # types 0 1 2 pure, 3 = (0, 1), 4 = (1, 2)
    assert d[0, 1] == 2 and d[0, 3] == 1 and d[1, 3] == 1 and d[1, 4] == 1 and d[0, 4] == 2 and d[2, 3] == 2 and d[3, 4] == 1
    typ = np.full((3, 3, 3), 1, dtype=np.uint8)
    typ[1, 1, 1] = 0
    typ[0, 1, 1] = pn.OFF                                               # a hole next to the centre
    typ[1, 1, 2] = 3
    cnt = pn.neighbour_counts(typ, 3)
    assert cnt[:, 0, 1, 1, 1].tolist() == [2, 4, 3] and cnt[:, 1, 1, 1, 1].tolist() == [0, 0, 1] and cnt[:, 3, 1, 1, 1].tolist() == [1, 2, 1]
    assert cnt[:, 1, 0, 0, 0].tolist() == [0, 0, 0]
    w = sn.axis_weights((1.0, 1.0, 3.0))
    assert pn.penalty(typ, 3, w, 0.3)[0, 1, 1, 1] == (0.3 * ((1.0 * 2 + 1.0 * 4) + (1.0 / 3.0) * 3)) * 0.5


@pytest.mark.parametrize("name", pn.CASES)
def test_fractions_sum_to_one_and_types_do_not_hang_on_rounding(name):
    """the inputs of tests/test_gpu_pve.py: the long-double restatement's smallest relative energy gap over all visits is >= 1e-9, fp64
    gives the same types, and the fractions are fractions"""
    c, r64 = staged(name)
    _, r80 = staged(name, np.longdouble)
    gaps, typ = pn.energy_gap(r80["E"], r80["om"], r80["live"], c["seg"], r80["w"], 0.3, 8)
    assert np.array_equal(typ, r80["mixeltype"])
    assert np.all(np.isinf(gaps[~c["om"]]))
    print("%s: N = %d, smallest relative gap %.3e, live %s" % (name, int(c["om"].sum()), gaps.min(), r64["live"].astype(int).tolist()))
    assert gaps.min() >= 1e-9
    assert np.array_equal(r64["mixeltype"], r80["mixeltype"]) and np.array_equal(r64["pveseg"], r80["pveseg"])
    assert np.abs(r64["pve"] - r80["pve"]).max() <= 1e-12
    p, om = r64["pve"], c["om"]
    assert np.all(p >= 0.0) and np.all(p[:, ~om] == 0.0)
    assert np.abs(p.sum(axis=0)[om] - 1.0).max() <= 2.0 ** -52
    assert np.all(r64["mixeltype"][~om] == pn.OFF) and np.all(r64["pveseg"][~om] == 0)
    assert np.array_equal(r64["pveseg"][om] - 1, np.argmax(p[:, om], axis=0))      # ties to the lowest class
    if c["dead"] is not None:
        K, j = c["K"], c["dead"]
        assert not r64["live"][j] and not r64["live"][K + j] and not r64["live"][K + j - 1]
        assert np.all(np.isinf(r64["E"][j][om])) and np.all(p[j] == 0.0)


def test_dead_classes_and_equal_means_kill_mixtures():
    mu, var, pi = np.array([500.0, 800.0, 1100.0]), np.array([400.0, 900.0, 1600.0]), np.array([0.3, 0.3, 0.4])
    assert pn.consts(mu, var, pi)[2].tolist() == [True] * 5
    assert pn.consts(mu, var, np.array([0.3, 0.0, 0.7]))[2].tolist() == [True, False, True, False, False]
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert pn.consts(mu, np.array([400.0, 900.0, bad]), pi)[2].tolist() == [True, True, False, True, False]
    assert pn.consts(np.array([500.0, 500.0, 1100.0]), var, pi)[2].tolist() == [True, True, True, False, True]
    assert pn.consts(np.array([800.0, 500.0, 1100.0]), var, pi)[2].tolist() == [True, True, True, False, True]
    a, h, live, tab = pn.consts(mu, var, np.array([0.3, 0.0, 0.7]))
    assert a[1] == 0.0 and h[1] == 0.0 and np.all(tab == 0.0)
    a, h, live, tab = pn.consts(mu, var, pi)
    assert tab.shape == (2, 64, 3) and np.all(np.diff(tab[0, :, 0]) < 0) and tab[0, 0, 0] < 800.0 and tab[0, -1, 0] > 500.0
    assert abs(tab[1, 31, 0] - (0.4921875 * 800.0 + 0.5078125 * 1100.0)) <= 1e-12


def test_with_all_types_dead_the_fractions_are_the_labels():
    rng = np.random.default_rng(3)
    shape = (4, 5, 6)
    seg = rng.integers(0, 4, size=shape).astype(np.uint8)
    prob = np.zeros((3,) + shape)                                        # no class has weight
    r = pn.partial_volume(rng.uniform(400.0, 1200.0, size=shape), seg, prob)
    assert not r["live"].any()
    for k in range(3):
        assert np.array_equal(r["pve"][k], (seg == k + 1).astype(np.float64))
    assert np.array_equal(r["pveseg"], seg) and np.array_equal(r["mixeltype"], np.where(seg == 0, pn.OFF, seg - 1))
    assert np.all(r["classes_lin"] == 0.0)
    c, one = staged("one")                                              # a single voxel: its class has no variance
    assert c["seg"].tolist() == [[[1]]] and not one["live"].any() and one["pve"].reshape(-1).tolist() == [1.0, 0.0, 0.0]


def test_the_fractions_beat_the_hard_labels_on_the_phantom():
    v, f = pn.phantom()
    res = sn.tissue_segment(v, None, (1.0, 1.0, 1.0))
    r = pn.partial_volume(v, res["seg"], res["prob"])
    mixed = f.max(axis=0) < 0.95
    hard = np.stack([res["seg"] == k + 1 for k in range(3)]).astype(np.float64)
    e_hard, e_pve = float(np.abs(hard - f)[:, mixed].mean()), float(np.abs(r["pve"] - f)[:, mixed].mean())
    print("%d truly mixed voxels of %d: mean absolute error of the hard labels %.3f, of the partial-volume model %.3f"
          % (int(mixed.sum()), mixed.size, e_hard, e_pve))
    assert mixed.sum() > 1000 and e_pve < e_hard


def test_drivers_refuse_a_bad_segment_before_any_device_work():
    motor = importlib.import_module(PKG + ".motor")
    data, mask, TE = np.ones((4, 4, 2, 8)), np.ones((4, 4, 2)), 10.0 * np.arange(1, 9)
    args = (mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    vox = (1.0, 1.0, 2.0)
    for bad in ("maybe", "PVE", 1, None):
        with pytest.raises(ValueError, match="segment must be"):
            motor.recon_met2_arrays(data, *args, segment=bad)
    with pytest.raises(ValueError, match="segment='pve' needs bias_correct"):
        motor.recon_met2_arrays(data, *args, segment="pve")
    with pytest.raises(ValueError, match="needs bias_correct"):
        motor.recon_met2_arrays(data, *args, segment="pve", bias_correct="no", voxel_size=vox)
    with pytest.raises(ValueError, match="distributed"):
        motor.recon_met2_arrays(data, *args, segment="pve", bias_correct="yes", voxel_size=vox, distributed=True)
    with pytest.raises(ValueError, match="voxel_size"):
        motor.recon_met2_arrays(data, *args, segment="pve", bias_correct="yes")
    with pytest.raises(ValueError, match="segment='yes' needs bias_correct='yes': the bias-corrected map is what is segmented"):
        motor._segment_check("yes", "no", False)                        # 'yes' keeps its messages
    with pytest.raises(ValueError, match="segment='yes' does not go with distributed=True: the map is complete only after the gather"):
        motor._segment_check("yes", "yes", True)
    assert motor._segment_check("pve", "yes", False) is True and motor._segment_check("no", "no", False) is False
    for f in (motor.recon_met2_arrays, motor.motor_recon_met2):
        assert inspect.signature(f).parameters["segment"].default == "no"
    sig = inspect.signature(motor.partial_volume_filter).parameters
    assert [sig[k].default for k in ("n_class", "beta", "beta_pv", "n_outer", "n_em", "n_icm", "seg", "prob")] == [3, 0.1, 0.3, 4, 10, 8, None, None]
    with pytest.raises(ValueError, match="seg and prob go together"):
        motor.partial_volume_filter(np.ones((2, 2, 2)), seg=np.ones((2, 2, 2), dtype=np.uint8))


def test_segment_pve_adds_exactly_three_keys(monkeypatch):
    """through the drivers' argument checking only: the fit and the three filters are stand-ins that touch no device.  With segment='pve' the
    partial-volume maps are made after the segmentation, from the corrected map and the segmentation's labels and posteriors, and the result
    gains three keys over segment='yes'; 'yes' and 'no' add none of them and do not call the filter"""
    motor = importlib.import_module(PKG + ".motor")
    data, mask, TE = np.ones((4, 4, 2, 8)), np.ones((4, 4, 2)), 10.0 * np.arange(1, 9)
    args = (mask, TE, 3000.0, "X2", "L2", "brute-force", 40.0)
    vox = (1.0, 1.0, 2.0)
    calls = []

    def fit(*a, **k):
        return {"TWC": np.full((4, 4, 2), 2.0), "MWF": np.zeros((4, 4, 2))}

    def bias(vol, mask, voxel_size, device=0, return_field=False, **k):
        calls.append("bias")
        return vol / 2.0, np.full(vol.shape, 2.0), None

    def segment(vol, mask, voxel_size, device=0, **k):
        calls.append("segment")
        return np.full(vol.shape, 2, dtype=np.uint8), np.full((3,) + vol.shape, 0.25), None

    def pve(vol, mask=None, voxel_size=(1, 1, 1), device=0, seg=None, prob=None, **k):
        calls.append("pve")
        assert np.all(vol == 1.0) and tuple(voxel_size) == vox           # the corrected map
        assert np.all(seg == 2) and np.all(prob == 0.25) and not k       # the segmentation's own outputs, the defaults otherwise
        return np.ones((3,) + vol.shape), np.ones(vol.shape, dtype=np.uint8), np.zeros(vol.shape, dtype=np.uint8), None

    monkeypatch.setattr(motor, "_recon_multi_device", fit)
    monkeypatch.setattr(motor, "bias_field_filter", bias)
    monkeypatch.setattr(motor, "tissue_segment_filter", segment)
    monkeypatch.setattr(motor, "partial_volume_filter", pve)
    new = ["TWC_mixeltype", "TWC_pve", "TWC_pveseg"]
    assert sorted(motor.recon_met2_arrays(data, *args, segment="no")) == ["MWF", "TWC"] and not calls
    with_bias = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="no")
    assert sorted(with_bias) == ["MWF", "TWC", "TWC_bias"] and calls == ["bias"]
    del calls[:]
    yes = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="yes")
    assert calls == ["bias", "segment"] and sorted(yes) == ["MWF", "TWC", "TWC_bias", "TWC_prob", "TWC_seg"]
    del calls[:]
    got = motor.recon_met2_arrays(data, *args, bias_correct="yes", voxel_size=vox, segment="pve")
    assert calls == ["bias", "segment", "pve"]
    assert sorted(got) == sorted(list(yes) + new)
    for k in yes:
        assert np.array_equal(got[k], yes[k])
    assert got["TWC_pve"].shape == (3, 4, 4, 2) and got["TWC_pveseg"].dtype == np.uint8 and got["TWC_mixeltype"].dtype == np.uint8


def test_bad_degibbs_and_bias_options_are_refused_before_any_device_work(monkeypatch):
    """the degibbs and bias_correct checks sit in the drivers' one resolver, before gibbs_filter and brain_mask_filter run"""
    motor = importlib.import_module(PKG + ".motor")
    filters = importlib.import_module(PKG + ".filters")

    def touched(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(motor, "lib", touched)
    monkeypatch.setattr(filters, "lib", touched)
    monkeypatch.setattr(motor, "gibbs_filter", touched)
    monkeypatch.setattr(motor, "brain_mask_filter", touched)
    data, mask, TE = np.ones((8, 8, 8, 8)), np.ones((8, 8, 8)), 10.0 * np.arange(1, 9)
    with pytest.raises(ValueError, match="bias_correct must be 'no' or 'yes'"):
        motor.recon_met2_arrays(data, mask, TE, 3000.0, degibbs="yes", bias_correct="maybe")
    with pytest.raises(ValueError, match=r"bias_correct='yes' needs voxel_size=\(dx, dy, dz\) in mm"):
        motor.recon_met2_arrays(data, mask, TE, 3000.0, degibbs="yes", bias_correct="yes")
    with pytest.raises(ValueError, match="degibbs must be 'no', 'yes' or '3d'"):
        motor.recon_met2_arrays(data, None, TE, 3000.0, degibbs="sometimes", brain_mask="yes", voxel_size=(1, 1, 1))


def test_both_drivers_take_the_same_options():
    motor = importlib.import_module(PKG + ".motor")
    arrays = [("data", None), ("mask", None), ("TE_array", None), ("TR", None), ("reg_method", "X2"), ("reg_matrix", "L2"),
              ("FA_method", "brute-force"), ("myelin_T2", 40.0), ("fa_index", None), ("device", 0), ("plan", None), ("denoise", "None"),
              ("prepared", False), ("FA_smooth", "no"), ("distributed", False), ("return_prepared", False), ("devices", None), ("bootstrap", None),
              ("degibbs", "no"), ("bias_correct", "no"), ("voxel_size", None), ("brain_mask", "no"), ("segment", "no"), ("tissue_stats", "no"),
              ("pve_threshold", 0.9), ("rician", "no"), ("rician_sigma", None), ("rician_iters", 3), ("slice_profile", None)]
    on_disk = [("TE_array", None), ("path_to_data", None), ("path_to_mask", None), ("path_to_save_data", None), ("TR", None), ("reg_method", None),
               ("reg_matrix", None), ("denoise", None), ("FA_method", None), ("FA_smooth", None), ("myelin_T2", None), ("num_cores", -1),
               ("device", 0), ("devices", None), ("bootstrap", None), ("degibbs", "no"), ("bias_correct", "no"), ("brain_mask", "no"),
               ("segment", "no"), ("tissue_stats", "no"), ("pve_threshold", 0.9), ("rician", "no"), ("rician_sigma", None), ("rician_iters", 3),
               ("slice_profile", None)]
    signature = lambda f: [(k, None if p.default is inspect.Parameter.empty else p.default) for k, p in inspect.signature(f).parameters.items()]
    assert signature(motor.recon_met2_arrays) == arrays
    assert signature(motor.motor_recon_met2) == on_disk
    for name, default in on_disk[[k for k, _ in on_disk].index("devices"):]:
        assert (name, default) in arrays, name


def test_the_device_list_leg_builds_one_plan_for_its_tail(monkeypatch):
    """devices=[...] with a bootstrap and tissue statistics: the post-fit steps run once each, in order, on ONE plan made on devices[0],
    which is closed whatever a step does.  The fit, the plan and the steps are recorders that touch no device."""
    motor = importlib.import_module(PKG + ".motor")
    data, mask, TE = np.ones((4, 4, 2, 8)), np.ones((4, 4, 2)), 10.0 * np.arange(1, 9)
    steps, plans = [], []

    class Plan:
        def __init__(self, n_te, n_t2, n_fa, device=0, **k):
            self.shape, self.device, self.closed = (n_te, n_t2, n_fa), device, 0
            plans.append(self)

        def build_dictionary_epg(self, *a, **k):
            return self

        def set_penalty(self, *a, **k):
            return self

        def close(self):
            self.closed += 1

    def fit(*a, **k):
        return {"TWC": np.full((4, 4, 2), 2.0), "MWF": np.zeros((4, 4, 2)), "FA_index": np.zeros((4, 4, 2)), "data_prepared": data.copy()}

    def step(name, fail=False):
        def record(res, *a, **k):
            steps.append((name, [x for x in a if isinstance(x, Plan)]))
            if fail:
                raise RuntimeError(name + " failed")
        return record

    monkeypatch.setattr(motor, "_recon_multi_device", fit)
    monkeypatch.setattr(motor, "Met2Plan", Plan)
    monkeypatch.setattr(motor, "_bootstrap_into", step("bootstrap"))
    monkeypatch.setattr(motor, "_bias_last", step("bias"))
    monkeypatch.setattr(motor, "_segment_last", step("segment"))
    monkeypatch.setattr(motor, "_tissue_stats_last", step("tissue statistics"))
    kw = dict(bootstrap=dict(n_rep=2), bias_correct="yes", voxel_size=(1.0, 1.0, 2.0), segment="yes", tissue_stats="yes")
    res = motor.recon_met2_arrays(data, mask, TE, 3000.0, devices=[3, 5], **kw)
    assert [name for name, _ in steps] == ["bootstrap", "bias", "segment", "tissue statistics"]
    assert len(plans) == 1 and plans[0].closed == 1 and plans[0].device == 3 and plans[0].shape == (8, 60, 91)
    assert steps[0][1] == [plans[0]] and steps[3][1] == [plans[0]]       # the bootstrap and the statistics share it
    assert "data_prepared" not in res                                    # asked for by the tail only, not by the caller
    del steps[:], plans[:]
    monkeypatch.setattr(motor, "_segment_last", step("segment", fail=True))
    with pytest.raises(RuntimeError, match="segment failed"):
        motor.recon_met2_arrays(data, mask, TE, 3000.0, devices=[3, 5], **kw)
    assert [name for name, _ in steps] == ["bootstrap", "bias", "segment"] and len(plans) == 1 and plans[0].closed == 1
    del steps[:], plans[:]
    motor.recon_met2_arrays(data, mask, TE, 3000.0, devices=[3], bias_correct="yes", voxel_size=(1.0, 1.0, 2.0))
    assert [name for name, _ in steps] == ["bias"] and not plans          # no plan where nothing needs one
