#!/usr/bin/env python3
"""What the registration recovers when the numpy restatement of the cost drives it on the CPU (no device), written to
profiles/register_recovery.json:
    python3 scripts/register_recovery.py [--out FILE]
    python3 scripts/register_recovery.py --mi [--out FILE]      the mutual-information costs -> profiles/register_mi_recovery.json
Per end-to-end case of tests/tools/register_numpy.py (the 20 x 18 x 16 phantom at 2 mm, a moving image under a known transform): the mean
displacement in mm, over the fixed mask's voxels, between the estimated and the true transform, and the share of the fixed grid's voxels whose
resampled atlas label differs between the two.  tests/test_gpu_register.py takes its bounds from this file: twice each figure (the device run
may take another, equivalent path through a flat minimum), the displacement capped at one fixed voxel.
--mi: the four cases {rigid6, affine12} x {mi, nmi} of tests/tools/register_mi_numpy.py on the remapped phantom, with the histogram sized per
level (register.level_bins), and the rigid6 / mi case once more with 64 x 64 cells forced on every level: the case the rule is there for.  That
file is a record (DESIGN.md quotes it); the tests hold these cases to half a fixed voxel, not to a multiple of its figures."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
PKG = "multicomponent-t2-toolbox_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mi", action="store_true", help="the mutual-information cases, to profiles/register_mi_recovery.json")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "register_mi_recovery.json" if a.mi else "register_recovery.json")
    import register_numpy as gn
    reg = importlib.import_module(PKG + ".register")
    rs = importlib.import_module(PKG + ".resample")
    if a.mi:
        return main_mi(a, gn, reg, rs)
    rows = {"phantom": list(gn.PHANTOM_SHAPE), "voxel_mm": gn.PHANTOM_MM, "cap_mm": gn.CAP_MM, "cost_fn": "register_numpy.prepare (long double)",
            "cases": {}}
    for name in ("rigid6", "affine12"):
        true_world, dof, kind, (fx, fa, mv, ma, mask) = gn.e2e_case(name, reg)
        t0 = time.perf_counter()
        out = reg.register(fx, fa, mv, ma, dof=dof, cost=kind, cost_fn=gn.prepare, filters=gn.FILTERS)
        rows["cases"][name] = {"dof": dof, "cost": kind, "mean_displacement_mm": gn.mean_displacement(out["world"], true_world, mask, fa),
                               "mean_displacement_before_mm": gn.mean_displacement(reg.params_to_world([0] * 6, 6), true_world, mask, fa),
                               "label_share": gn.label_share(out["world"], true_world, fa, ma, rs.voxel_matrix), "final_cost": out["cost"],
                               "n_eval": sum(l["n_eval"] for l in out["levels"]), "seconds": time.perf_counter() - t0}
        print(name, json.dumps(rows["cases"][name]))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


def main_mi(a, gn, reg, rs):
    import numpy as np
    import register_mi_numpy as mn
    rows = {"phantom": list(gn.PHANTOM_SHAPE), "voxel_mm": gn.PHANTOM_MM, "bound_mm": gn.PHANTOM_MM / 2.0, "cost_fn": "register_mi_numpy.prepare (long double)",
            "histogram": "B x B per level, B = min(n_bins, max(4, integer cube root of n_included)), n_bins = 64", "cases": {}}

    def forced(fixed, fixed_bin, moving, kind, n_bins, min_overlap):       # 64 x 64 cells whatever the level
        b = reg.bin_intensity(fixed, 64)
        b[np.asarray(fixed_bin) < 0] = -1
        return mn.prepare(fixed, b, moving, kind, 64, min_overlap)

    for name, cost_fn in [(n, None) for n in mn.E2E_CASES] + [("rigid6_mi", forced)]:
        true_world, dof, kind, (fx, fa, mv, ma, mask) = mn.e2e_case(name, reg)
        bins = []

        def recording(fixed, fixed_bin, moving, kind_, n_bins, min_overlap):
            bins.append({"n_included": int((np.asarray(fixed_bin) >= 0).sum()), "bins": n_bins if cost_fn is None else 64})
            return (mn.prepare if cost_fn is None else cost_fn)(fixed, fixed_bin, moving, kind_, n_bins, min_overlap)

        t0 = time.perf_counter()
        out = reg.register(fx, fa, mv, ma, dof=dof, cost=kind, cost_fn=recording, filters=gn.FILTERS)
        key = name if cost_fn is None else name + "_64x64_on_every_level"
        rows["cases"][key] = {"dof": dof, "cost": kind, "levels": bins, "mean_displacement_mm": gn.mean_displacement(out["world"], true_world, mask, fa),
                              "mean_displacement_before_mm": gn.mean_displacement(reg.params_to_world([0] * 6, 6), true_world, mask, fa),
                              "label_share": gn.label_share(out["world"], true_world, fa, ma, rs.voxel_matrix), "final_cost": out["cost"],
                              "n_eval": sum(l["n_eval"] for l in out["levels"]), "seconds": time.perf_counter() - t0}
        print(key, json.dumps(rows["cases"][key]))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
