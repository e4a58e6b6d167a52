"""GPU tests of the Monte-Carlo study (csrc/met2_eval.hip, met2_amd.evaluate): the generator against the recipe (tests/eval_ref.py with
synth.epg_table at each voxel's exact flip angle), chunk invariance, the Rician noise, the metric and reduction kernels against eval_ref,
the reference's three tables (tests/golden/eval_tables_paper.json) within their statistical error, and determinism."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import eval_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PKG = "multicomponent-t2-toolbox_amd"
N_PAPER = 10000


@pytest.fixture(scope="module")
def ev():
    assert torch.cuda.is_available()
    importlib.import_module(PKG + "._build").build()
    return importlib.import_module(PKG + ".evaluate")


def study_plan(ev, nte, npc, nfa=1):
    pkg = importlib.import_module(PKG)
    T2s = ev.study_t2_grid(npc)
    plan = pkg.Met2Plan(nte, npc, nfa, device=0)
    alphas = np.array([150.0]) if nfa == 1 else np.linspace(90.0, 180.0, nfa)
    plan.build_dictionary_epg(T2s, 1000.0 * np.ones(npc), 10.0, alphas, 3000.0)
    return plan, T2s


def rel_rows(a, b):
    return np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)


@pytest.mark.parametrize("nte,npc", [(32, 60), (48, 120)])
def test_generator_matches_the_recipe(ev, nte, npc):
    plan, T2s = study_plan(ev, nte, npc)
    clean = ev.synth_two_lobe(plan, 256, seed=42, snr=None)
    noisy = ev.synth_two_lobe(plan, 256, seed=42, snr=(50.0, 150.0))
    torch.cuda.synchronize()
    tr = clean["truth"].cpu().numpy()
    data, d2, mwf = eval_ref.synth_clean(tr, nte, T2s)
    assert rel_rows(clean["data"].cpu().numpy(), data).max() < 1e-12
    assert rel_rows(clean["dist2"].cpu().numpy(), d2).max() < 1e-12
    np.testing.assert_allclose(tr[0], mwf, rtol=1e-12, atol=1e-15)
    # draws inside the reference's ranges; FA continuous, not on a 1-degree grid
    for row, (lo, hi) in ((6, (0.05, 0.25)), (1, (15, 35)), (2, (60, 90)), (4, (90, 180)), (7, (1, 3)), (8, (6, 12))):
        assert tr[row].min() >= lo and tr[row].max() < hi
    assert np.all(tr[3] == 1000.0) and np.all(np.isinf(tr[5]))
    assert np.mean(tr[4] != np.round(tr[4])) > 0.99
    # noise changes the echoes and SNR, nothing else
    trn = noisy["truth"].cpu().numpy()
    np.testing.assert_array_equal(np.delete(trn, 5, axis=0), np.delete(tr, 5, axis=0))
    assert trn[5].min() >= 50.0 and trn[5].max() < 150.0
    np.testing.assert_array_equal(noisy["dist2"].cpu().numpy(), clean["dist2"].cpu().numpy())
    assert not torch.equal(noisy["data"], clean["data"])
    plan.close()


def test_generator_chunk_invariance(ev):
    plan, _ = study_plan(ev, 32, 60)
    whole = ev.synth_two_lobe(plan, 300, seed=9, snr=(50.0, 150.0))
    parts = [ev.synth_two_lobe(plan, n, seed=9, snr=(50.0, 150.0), voxel_offset=o) for o, n in ((0, 77), (77, 150), (227, 73))]
    torch.cuda.synchronize()
    for k in ("data", "dist2"):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts], dim=0)), k
    assert torch.equal(whole["truth"], torch.cat([p["truth"] for p in parts], dim=1))
    other = ev.synth_two_lobe(plan, 300, seed=10, snr=(50.0, 150.0))
    assert not torch.equal(other["data"], whole["data"])
    plan.close()


def test_rician_noise_moments(ev):
    # at a fixed SNR of 20, M = |A + sigma (z1 + i z2)| with sigma = A_0 / 20: E M = sigma sqrt(pi/2) L_1/2(-nu), E M^2 = A^2 + 2 sigma^2,
    # nu = A^2 / (2 sigma^2).  Standardised per (voxel, echo), mean 0 and variance 1 within 5 standard errors.
    plan, _ = study_plan(ev, 32, 60)
    n = 4096
    clean = ev.synth_two_lobe(plan, n, seed=3, snr=None)["data"].cpu().double()
    noisy = ev.synth_two_lobe(plan, n, seed=3, snr=(20.0, 20.0))["data"].cpu().double()
    sg = clean[:, :1] / 20.0
    nu = clean ** 2 / (2 * sg ** 2)
    mean = sg * np.sqrt(np.pi / 2) * ((1 + nu) * torch.special.i0e(nu / 2) + nu * torch.special.i1e(nu / 2))
    var = clean ** 2 + 2 * sg ** 2 - mean ** 2
    z = ((noisy - mean) / torch.sqrt(var)).numpy().ravel()
    N = z.size
    assert abs(z.mean()) < 5 / np.sqrt(N), z.mean()
    assert abs(np.mean(z ** 2) - 1.0) < 5 * np.std(z ** 2) / np.sqrt(N), np.mean(z ** 2)
    plan.close()


@pytest.mark.parametrize("nte,npc", [(32, 60), (48, 120)])
def test_metric_and_reduce_kernels_match_eval_ref(ev, nte, npc):
    plan, T2s = study_plan(ev, nte, npc, nfa=91)
    plan.set_lambda_grid(ev.study_lambda_grid())
    n = 4096
    g = ev.synth_two_lobe(plan, n, seed=17, snr=(50.0, 150.0))
    fa, _, _ = plan.fa_bruteforce(g["data"])
    truth = g["truth"].cpu().numpy()
    d2 = g["dist2"].cpu().numpy()
    nnls_fie = None
    for label in ev.PAPER_METHODS:
        method, pen = ev.METHOD_SPEC[label]
        plan.set_penalty(pen)
        out = plan.fit(method, g["data"], fa_index=fa, want_lambda=method != "NNLS")
        pv = ev.voxel_metrics(plan, out["fsol"], g["dist2"])
        lam = out["lam"] if method != "NNLS" else None
        fie = pv[1].clone() if nnls_fie is None else nnls_fie
        agg = ev.reduce_metrics(pv, g["truth"], lam, fie)
        nnls_fie = fie
        got = pv.cpu().numpy()
        fs = out["fsol"].cpu().numpy()
        want = np.stack([eval_ref.voxel_metrics(fs[v], d2[v], T2s) for v in range(n)], axis=1)
        np.testing.assert_array_equal(got[5], want[5], err_msg=label + " peaks")
        for k in (0, 1, 2, 3, 4, 6, 7, 8):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=1e-15, err_msg="%s %s" % (label, ev.FIELDS[k]))
        ref = eval_ref.reduce_metrics(want, truth, None if lam is None else lam.cpu().numpy(), fie.cpu().numpy())
        np.testing.assert_allclose(agg, ref, rtol=1e-10, atol=1e-13, err_msg=label + " aggregates")
    plan.close()


def bootstrap_se(ev, pvd, methods, B=200, seed=0):
    """standard errors of the 15 aggregates of every method from a voxel bootstrap of the per-voxel arrays (eval_ref.reduce_metrics)"""
    rng = np.random.default_rng(seed)
    tr = pvd["truth"]
    truth = np.stack([tr[k] for k in ev.TRUTH])
    n = truth.shape[1]
    pv = {m: np.stack([pvd[m][f] for f in ev.FIELDS]) for m in pvd if m not in ("truth", "fa_index")}
    fie = pv["1. NNLS"][1]
    reps = np.zeros((B, len(methods), 15))
    for b in range(B):
        i = rng.integers(0, n, n)
        for k, m in enumerate(methods):
            reps[b, k] = eval_ref.reduce_metrics(pv[m][:, i], truth[:, i], pvd[m]["lam"][i], fie[i])
    return reps.std(axis=0, ddof=1)


@pytest.mark.parametrize("band", ["50_150", "150_300", "inf"])
def test_paper_tables(ev, band):
    with open(os.path.join(GOLDEN, "eval_tables_paper.json")) as f:
        fx = json.load(f)
    b = fx["bands"][band]
    snr = None if b["snr"] is None else tuple(b["snr"])
    res = ev.evaluate_methods(n_voxels=N_PAPER, snr=snr, seed=2024, per_voxel=True)
    assert res.methods == ev.PAPER_METHODS
    ours = np.concatenate([res.errors, res.regularization], axis=1)
    paper = np.concatenate([np.asarray(b["errors"]), np.asarray(b["regularization_csv"])], axis=1)
    se = bootstrap_se(ev, res.per_voxel, res.methods) * np.sqrt(1.0 + N_PAPER / fx["n_voxels"])
    cols = ev.ERROR_COLUMNS + ev.REG_COLUMNS
    bad = []
    for r, m in enumerate(res.methods):
        for c, col in enumerate(cols):
            if not abs(ours[r, c] - paper[r, c]) <= 4.0 * se[r, c]:
                bad.append("%s %s: ours %.6g paper %.6g se %.3g (%.1f se)" % (m, col, ours[r, c], paper[r, c], se[r, c],
                                                                             abs(ours[r, c] - paper[r, c]) / max(se[r, c], 1e-300)))
    assert not bad, "\n".join(bad)
    assert np.all(res.regularization[0] == 0.0)
    # the paper's ordering: where the paper's worst row of MAE, RMSE, cRMSE or MAE-S is NNLS, ours is NNLS too.  (NNLS has the worst MAE
    # at SNR 50-150 and without noise; at 150-300 the paper's worst MAE is L-curve-L1's, 0.0550 against NNLS's 0.0517.)
    pe = np.asarray(b["errors"])
    checked = 0
    for c in (0, 2, 3, 10):
        if np.argmax(pe[:, c]) == 0:
            assert np.argmax(res.errors[:, c]) == 0, ev.ERROR_COLUMNS[c]
            checked += 1
    assert checked >= 3


def test_determinism_and_chunking(ev):
    a = ev.evaluate_methods(n_voxels=6000, snr=(50.0, 150.0), seed=5, chunk=6000, per_voxel=True)
    b = ev.evaluate_methods(n_voxels=6000, snr=(50.0, 150.0), seed=5, chunk=6000)
    c = ev.evaluate_methods(n_voxels=6000, snr=(50.0, 150.0), seed=5, chunk=2500, per_voxel=True)
    np.testing.assert_array_equal(a.errors, b.errors)
    np.testing.assert_array_equal(a.regularization, b.regularization)
    for m in ev.PAPER_METHODS:
        for f in ev.FIELDS + ("lam",):
            np.testing.assert_array_equal(a.per_voxel[m][f], c.per_voxel[m][f], err_msg="%s %s" % (m, f))
    np.testing.assert_array_equal(a.errors, c.errors)


def test_evaluate_at_120_bins_is_chunk_invariant(ev):
    # L-curve at n_t2 > 64 is fitted in slices of 4 096 voxels (evaluate._LCURVE_SLICE): chunks above and below that give the same bits
    m = ("1. NNLS", "7. Lcurve-L2")
    a = ev.evaluate_methods(n_voxels=5000, snr=(50.0, 150.0), seed=8, nte=48, npc=120, methods=m, chunk=5000, per_voxel=True)
    c = ev.evaluate_methods(n_voxels=5000, snr=(50.0, 150.0), seed=8, nte=48, npc=120, methods=m, chunk=1700, per_voxel=True)
    for f in ev.FIELDS + ("lam",):
        np.testing.assert_array_equal(a.per_voxel["7. Lcurve-L2"][f], c.per_voxel["7. Lcurve-L2"][f])
    np.testing.assert_array_equal(a.errors, c.errors)


def test_write_tables_from_a_run(ev, tmp_path):
    res = ev.evaluate_methods(n_voxels=2000, snr=(50.0, 150.0), seed=1)
    res.write_tables(str(tmp_path))
    txt = (tmp_path / "table_errors.txt").read_text().splitlines()
    assert len(txt) == 12 and txt[0].split()[:3] == ["Method", "1.", "MAE"]
    csv = (tmp_path / "table_errors.csv").read_text().splitlines()
    assert len(csv) == 10 and all(len(r.split(",")) == 14 for r in csv)
    reg = (tmp_path / "table_regularization.csv").read_text().splitlines()
    assert reg[0] == "1. NNLS               ,0,0" and len(reg) == 10
