"""Transcribes the reference's Monte-Carlo tables into eval_tables_paper.json (labels and numbers only):

    python tests/golden/make_eval_tables.py <Paper_Comparison/Results> [out.json]

Reads, for each SNR band, All_methods_10000iters/table_errors.txt and table_regularization.txt (the tables the paper is built on), and the
full-precision lambdas of table_regularization.csv; records the sha256 of all four files so that a test can check that
evaluate.EvalResult.write_tables reproduces their layout byte for byte.  Parses text only: imports nothing from the reference."""
import hashlib
import json
import os
import sys

BANDS = {"50_150": ("SNRs_50_150", [50.0, 150.0]), "150_300": ("SNRs_150_300", [150.0, 300.0]), "inf": ("SNRs_Inf", None)}
FILES = ("table_errors.txt", "table_errors.csv", "table_regularization.txt", "table_regularization.csv")


def parse_txt(text):
    """tabulate's 'simple' layout: header line, dash line, rows of '<label>  <number> ...' (labels may hold one space: '1. NNLS')."""
    lines = text.splitlines()
    rows = []
    for ln in lines[2:]:
        parts = ln.split()
        k = next(i for i, p in enumerate(parts) if i > 0 and _isnum(p) and not parts[i - 1].endswith("."))
        rows.append([" ".join(parts[:k])] + [float(p) for p in parts[k:]])
    return rows


def _isnum(s):
    try:
        float(s)
        return True
    except ValueError:
        return False


def main(results, out):
    bands = {}
    for key, (sub, snr) in BANDS.items():
        d = os.path.join(results, sub, "All_methods_10000iters")
        raw = {f: open(os.path.join(d, f), "rb").read() for f in FILES}
        err = parse_txt(raw["table_errors.txt"].decode())
        reg = parse_txt(raw["table_regularization.txt"].decode())
        reg_csv = [ln.split(",") for ln in raw["table_regularization.csv"].decode().splitlines()]
        err_csv = [ln.split(",") for ln in raw["table_errors.csv"].decode().splitlines()]
        bands[key] = {
            "snr": snr,
            "methods": [r[0] for r in err],
            "errors": [r[1:] for r in err],
            "regularization": [r[1:] for r in reg],
            "errors_csv": [[float(x) for x in r[1:]] for r in err_csv],
            "regularization_csv": [[float(x) for x in r[1:]] for r in reg_csv],
            "sha256": {f: hashlib.sha256(raw[f]).hexdigest() for f in FILES},
        }
        assert [r[0] for r in reg] == bands[key]["methods"], (key, [r[0] for r in reg])
        assert all(len(r) == 13 for r in bands[key]["errors"]) and all(len(r) == 2 for r in bands[key]["regularization"])
    doc = {"source": "scripts_synthetic_data_evaluation/Paper_Comparison/Results/<band>/All_methods_10000iters (10 000 voxels per band)",
           "error_columns": ["1. MAE", "2. MARE", "3. RMSE", "4. cRMSE", "5. RMSRE", "6. U95", "7. MBE", "8. R", "9. GMARE", "10. MAE-k",
                             "11. MAE-S", "12. MJSD-S", "13. MWD-S"],
           "regularization_columns": ["mean Lambda", "STD"], "n_voxels": 10000, "bands": bands}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_tables_paper.json"))
