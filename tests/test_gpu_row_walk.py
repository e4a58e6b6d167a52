"""The half-wave model signal (csrc/nnls_wave.hpp: model_signal at one bin per lane and nTE <= 32) gives the BITS of the loop it replaces: its two
summation chains run on the two half waves (lane e: positions p, p + 2, ...; lane 32 + e: p + 1, p + 3, ... of the same echo) and are added
through one lane exchange -- the same FMAs on the same operands in the same order in every lane that contributes to an output.

Each case is fitted in two fresh child processes, each under its own time limit: one on the default path, one with MET2_ROWWALK_REF=1 (the
loops of before); every output of every voxel must be array_equal.  The cases: X2/L2 at 32 x 60 (nTE = 32: the half-wave form's upper
edge); nTE = 31 and 33 (the last shape inside the half-wave form, and the first outside it: 33 takes the old loop whatever the switch says);
X2/I (another distribution of passive sets: sizes 4 q + 1, 4 q + 2, 4 q + 3 and beyond 32 are asserted); nT2 = 61 and 64 (up to a
full wave of bins); the L-curve with L1 and T2SPARC (the other one-bin-per-lane kernels); X2/L2 on a voxel list
with 16 flip angles (row bases differ per voxel); and X2/L2 at 48 x 120 (two bins per lane: those kernels have no half-wave form and must be equal
with and without the switch).

The switch reaches fit_kernel and its spill-over kernels, as MET2_SUBST_REF does.  The wave reductions' cross-row stage (csrc/wave_ops.hpp)
has no switch: it is compared against the parent build's dumped outputs (profiles/rowwalk_ab.txt)."""
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

PKG = "multicomponent-t2-toolbox_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FIELDS = ("fsol", "sig", "reg", "lam", "maps", "status")
SEED = 20260102           # bench.py's
NFA = 16                  # flip angles of the per-voxel FA case
# name: (method, penalty, nTE, nT2, voxels, per-voxel flip-angle indices)
CASES = {"X2-L2": ("X2", "L2", 32, 60, 4096, False),
         "X2-L2-nte31": ("X2", "L2", 31, 60, 1024, False),
         "X2-L2-nte33": ("X2", "L2", 33, 60, 1024, False),
         "X2-I": ("X2", "I", 32, 60, 1024, False),
         "X2-L2-nt2-61": ("X2", "L2", 32, 61, 1024, False),
         "X2-L2-nt2-64": ("X2", "L2", 32, 64, 1024, False),
         "L_curve-L1": ("L_curve", "L1", 32, 60, 1024, False),
         "T2SPARC-L2": ("T2SPARC", "L2", 32, 60, 1024, False),
         "X2-L2-FA": ("X2", "L2", 32, 60, 2048, True),
         "X2-L2-48x120": ("X2", "L2", 48, 120, 512, False)}


def _run(name, out_path=None):
    """fit the case on cuda:0 under the environment as it is; returns the outputs as numpy"""
    import torch
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    method, pen, nte, nt2, nvox, brute = CASES[name]
    T2s = synth.t2_grid(nt2)
    alphas = np.linspace(90.0, 180.0, NFA) if brute else np.array([150.0])
    plan = pkg.Met2Plan(nte, nt2, alphas.size, device=0)
    plan.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, alphas, 3000.0).set_penalty(pen, T2s)
    data, fa, _ = synth.make_voxels(nvox, nte=nte, seed=SEED, fa_deg=150.0, fa_values=alphas if brute else None, device="cuda:0")
    out = plan.fit(method, data, fa_index=fa if brute else None, want_lambda=True)
    torch.cuda.synchronize()
    res = {k: out[k].cpu().numpy() for k in FIELDS}
    if brute:
        assert np.unique(fa.cpu().numpy()).size == NFA          # several dictionaries are hit
    plan.close()
    if out_path:
        np.savez(out_path, **res)
    return res


def _child(name, path, ref):
    """the case in a fresh process with its own time limit, on the half waves or (MET2_ROWWALK_REF=1) on the loop of before"""
    env = {k: v for k, v in os.environ.items() if k != "MET2_ROWWALK_REF"}
    if ref:
        env["MET2_ROWWALK_REF"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), name, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    z = np.load(path)
    return {k: z[k] for k in FIELDS}


@pytest.mark.parametrize("name", list(CASES))
def test_row_walks_give_the_reference_loops_bits(name):
    with tempfile.TemporaryDirectory() as tmp:
        got = _child(name, os.path.join(tmp, "new.npz"), False)
        ref = _child(name, os.path.join(tmp, "ref.npz"), True)
    nvox = CASES[name][4]
    size = np.count_nonzero(got["fsol"], axis=1)             # the final passive set of a voxel (a passive bin at exactly zero is not counted)
    print("MEASURED %s: %d voxels, final passive sets %d..%d bins (mean %.1f), sizes mod 4: %s, %d beyond 32"
          % (name, nvox, size.min(), size.max(), size.mean(), [int((size % 4 == r).sum()) for r in range(4)], int((size > 32).sum())))
    for k in FIELDS:
        assert got[k].shape == ref[k].shape and got[k].shape[-1 if k == "maps" else 0] == nvox
        assert np.array_equal(got[k], ref[k], equal_nan=True), "%s: %s differs in %d entries" % (name, k, int((got[k] != ref[k]).sum()))
    assert np.isfinite(got["fsol"]).all() and (size > 0).any()
    if name == "X2-I":
        for r in (1, 2, 3):
            assert (size % 4 == r).any()                     # every tail of the walk in fours
        assert (size > 32).any()                             # sets beyond the half wave


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    _run(sys.argv[1], sys.argv[2])
