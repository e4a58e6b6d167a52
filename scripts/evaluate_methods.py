"""The reference's Monte-Carlo accuracy study for one SNR band on the GPU (met2_amd.evaluate.evaluate_methods), written as the reference
writes it: table_errors.{txt,csv} and table_regularization.{txt,csv}.

    python scripts/evaluate_methods.py --snr 50 150 --n 10000 --out DIR
    python scripts/evaluate_methods.py --snr inf --n 10000 --nte 48 --npc 120 --out DIR
    python scripts/evaluate_methods.py --snr 50 150 --n 10000 --rician iterative --out DIR    (every fit with the Rician noise floor taken out)"""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "multicomponent-t2-toolbox_amd"


def main(argv=None):
    ev = importlib.import_module(PKG + ".evaluate")
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--snr", nargs="+", default=["50", "150"], help="LO HI, or inf for the noise-free band")
    ap.add_argument("--n", type=int, default=10000, help="voxels (default 10000, as the reference)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--nte", type=int, default=32)
    ap.add_argument("--npc", type=int, default=60)
    ap.add_argument("--methods", nargs="+", default=None, help="row labels (default: the ten of the paper), e.g. '1. NNLS' '4. X2-L2'")
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rician", choices=["iterative"], default=None, help="fit through Met2Plan.fit_rician (sigma estimated per voxel)")
    ap.add_argument("--rician-iters", type=int, default=3)
    ap.add_argument("--out", required=True, help="directory for the four table files")
    a = ap.parse_args(argv)
    if len(a.snr) == 1 and a.snr[0].lower() == "inf":
        snr = None
    elif len(a.snr) == 2:
        snr = (float(a.snr[0]), float(a.snr[1]))
    else:
        ap.error("--snr takes LO HI or inf")
    importlib.import_module(PKG + "._build").build()
    t = time.perf_counter()
    res = ev.evaluate_methods(n_voxels=a.n, snr=snr, seed=a.seed, nte=a.nte, npc=a.npc, methods=tuple(a.methods or ev.PAPER_METHODS),
                              chunk=a.chunk, device=a.device, rician=a.rician, rician_iters=a.rician_iters)
    wall = time.perf_counter() - t
    res.write_tables(a.out)
    print(res.error_table())
    print()
    print(res.regularization_table())
    print("\n%d voxels x %d methods in %.2f s; tables in %s" % (a.n, len(res.methods), wall, a.out))


if __name__ == "__main__":
    main()
