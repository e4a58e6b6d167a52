#!/usr/bin/env python3
"""What the non-linear registration recovers when the numpy restatement of its stages drives it on the CPU (no device), written to
profiles/warp_recovery.json:
    python3 scripts/warp_recovery.py [--out FILE]
The recovery case of tests/tools/warp_numpy.py (the 20 x 18 x 16 phantom at 2 mm; the moving image is the phantom under a smooth field of up to
3 mm), in the same contrast and inverted: the mean error |u + d(P + u)| in mm over fixed > 0.05 before and after, the metric's first and last
value per level, and the same two runs with the plain clamped gradient in place of the rule's -- the record of why the rule looks at `inside`.
tests/test_gpu_warp.py holds the device run to within a stated margin of error_after_mm."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_recovery.json"))
    a = ap.parse_args()
    import numpy as np
    import register_numpy as gn
    import warp_numpy as wn
    warp = importlib.import_module(PKG + ".warp")
    rows = {"phantom": list(gn.PHANTOM_SHAPE), "voxel_mm": gn.PHANTOM_MM, "stages": "warp_numpy.stages (fp64)", "filters": "register_numpy.FILTERS",
            "options": {k: list(v) if isinstance(v, tuple) else v for k, v in wn.RECOVERY_OPTIONS.items()}, "required_ratio": wn.RECOVERY_RATIO}
    for key, inverted, plain in (("same_contrast", False, False), ("inverted", True, False), ("same_contrast_plain_gradient", False, True),
                                 ("inverted_plain_gradient", True, True)):
        fixed, moving, aff = wn.recovery_pair(inverted)
        t0 = time.perf_counter()
        out = warp.register(fixed, aff, moving, aff, None, stages=wn.stages(np.float64, plain), filters=gn.FILTERS, **wn.RECOVERY_OPTIONS)
        before, after = wn.recovery_error(np.zeros(fixed.shape + (3,)), fixed, aff), wn.recovery_error(out["disp"], fixed, aff)
        rows[key] = {"error_before_mm": before, "error_after_mm": after, "ratio": after / before,
                     "levels": [{"shape": list(L["shape"]), "iters": L["iters"], "metric_first": L["metric"][0], "metric_last": L["metric"][-1],
                                 "metric_max": max(L["metric"])} for L in out["levels"]], "seconds": time.perf_counter() - t0}
        print(key, json.dumps(rows[key]))
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
