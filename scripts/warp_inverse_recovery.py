"""The label round trip of tests/test_gpu_warp_inverse.py on the CPU, with the numpy restatement (tests/tools/warp_inverse_numpy.py in fp64):
warp_numpy.atlas_case()'s labels are pushed onto the maps' grid through (A, u), u the true field, and pulled back through (B, v), v the
fixed-point inverse after 20 steps.  The share of the labelled voxels that come back with their own label is what the device test holds the
library to (minus 0.5 % of the labelled voxels for ties at label borders).  No device is needed.
    python scripts/warp_inverse_recovery.py [profiles/warp_inverse_recovery.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import warp_numpy as wn                                            # noqa: E402
import warp_inverse_numpy as wi                                    # noqa: E402

N_ITER = 20


def main(path):
    lab, la, fa, A, u, truth = wi.round_trip_inputs()
    inv = wi.invert(u, A, lab.shape, N_ITER, np.float64)
    back = wn.warp_labels(truth, inv["B"], inv["disp"])
    s, n = wi.label_share(back, lab)
    det, folds = wi.jacobian(u, 1.0, np.float64)
    out = {"share_recovered": s, "n_labelled": n, "n_iter": N_ITER, "residual_last": float(inv["residual"][-1]), "inside_share": float(inv["inside"].mean()),
           "jacobian_min": float(det.min()), "jacobian_max": float(det.max()), "n_nonpositive": folds, "margin_share": 0.005,
           "reference": "tests/tools/warp_inverse_numpy.py in fp64 on warp_numpy.atlas_case()"}
    print(json.dumps(out))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "warp_inverse_recovery.json"))
