"""The packed leg of the warm re-factorisation (csrc/nnls_wave.hpp, refactor_rowwise<..., PACK>: four pivot rows per step on the wave's two
halves while 4 <= k <= 32, one bin per lane) gives the BITS of the pair loop: every row keeps its order of summation.

Each case is fitted in this process with the default path and in a child process with MET2_REFAC_PAIR=1 (the pair loop only); both run
with MET2_REFAC_COUNT=1, which makes the fit kernels count the re-factorisations that took the packed leg (met2_refac_packed_calls).  Every
output of every voxel must be array_equal, the default run must have taken the packed leg and the child must not have.  A third fit in
this process without the counter must give the same bits again."""
import ctypes as C
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
# (name, method, penalty, voxels, per-voxel flip-angle indices)
CASES = [("X2-L2", "X2", "L2", 65536, False), ("X2-I", "X2", "I", 65536, False), ("L_curve-L1", "L_curve", "L1", 8192, False),
         ("X2-L2-FA", "X2", "L2", 65536, True)]


def _run(name, out_path=None):
    """fit the case on cuda:0 (32 x 60) under the environment as it is; returns (outputs as numpy, packed calls counted)"""
    import torch
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    lib = importlib.import_module(PKG + "._lib")
    _, method, pen, nvox, brute = [c for c in CASES if c[0] == name][0]
    nte, nt2 = 32, 60
    T2s = synth.t2_grid(nt2)
    alphas = np.linspace(90.0, 180.0, NFA) if brute else np.array([150.0])
    plan = pkg.Met2Plan(nte, nt2, alphas.size, device=0)
    plan.build_dictionary_epg(T2s, 1000.0 * np.ones(nt2), 10.0, alphas, 3000.0).set_penalty(pen, T2s)
    data, fa, _ = synth.make_voxels(nvox, nte=nte, seed=SEED, fa_deg=150.0, fa_values=alphas if brute else None, device="cuda:0")
    calls = C.c_uint64(0)
    assert lib.lib().met2_refac_packed_calls(plan._h, C.byref(calls), 1) == 0       # reset
    out = plan.fit(method, data, fa_index=fa if brute else None, want_lambda=True)
    torch.cuda.synchronize()
    assert lib.lib().met2_refac_packed_calls(plan._h, C.byref(calls), 1) == 0
    res = {k: out[k].cpu().numpy() for k in FIELDS}
    if brute:
        assert np.unique(fa.cpu().numpy()).size == NFA          # several dictionaries are hit
    plan.close()
    if out_path:
        np.savez(out_path, calls=np.uint64(calls.value), **res)
    return res, int(calls.value)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_packed_leg_gives_the_pair_loops_bits(name, monkeypatch):
    monkeypatch.setenv("MET2_REFAC_COUNT", "1")
    monkeypatch.delenv("MET2_REFAC_PAIR", raising=False)
    got, calls = _run(name)
    nvox = got["reg"].shape[0]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "pair.npz")
        env = dict(os.environ, MET2_REFAC_PAIR="1", MET2_REFAC_COUNT="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), name, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1200)
        assert p.returncode == 0, p.stdout + p.stderr
        ref = np.load(path)
        ref_calls = int(ref["calls"])
        ref = {k: ref[k] for k in FIELDS}
    print("MEASURED %s: %d voxels, packed leg taken by %d re-factorisations (%.1f per voxel); pair-only child: %d"
          % (name, nvox, calls, calls / nvox, ref_calls))
    assert ref_calls == 0, ref_calls                    # the child ran the pair loop alone
    # the default run took the packed leg.  The floor: an X2 voxel re-factorises once per Brent evaluation (scipy's fminbound needs at least ~12 for
    # xatol 1e-5 on [0, 10]: the golden section alone would need 29) and the passive sets are 21-35 bins at the first abscissa, ~20 at the
    # last, so nearly every call has 4 <= k <= 32; the L-curve sweeps 50 grid points, most of them at large lambda (small sets)
    floor = 25 if name.startswith("L_curve") else 12
    assert calls >= floor * nvox, (calls, nvox, floor)
    for k in FIELDS:
        assert got[k].shape == ref[k].shape and got[k].shape[-1 if k == "maps" else 0] == nvox
        assert np.array_equal(got[k], ref[k], equal_nan=True), "%s: %s differs in %d entries" % (name, k, int((got[k] != ref[k]).sum()))
    # the shipped default (no counter) gives the same bits
    monkeypatch.delenv("MET2_REFAC_COUNT")
    plain, none = _run(name)
    assert none == 0
    for k in FIELDS:
        assert np.array_equal(plain[k], got[k], equal_nan=True), "%s without the counter: %s differs" % (name, k)


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    _run(sys.argv[1], sys.argv[2])
