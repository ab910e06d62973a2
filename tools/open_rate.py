"""Times pg_poly_open (csrc/opening.hpp) at 2^28 on random columns, warmed up: the prover's xi aggregate (20 distinct columns,
the first weight 1 as t_lo's is) and its xi omega aggregate (4 columns, weights 1, v', v'^2, v'^3).  One JSON line per aggregate:
ms median / min / max, the field multiplications per second and their share of the fr_mul ceiling (tools/fr_mul_bench.hip), and
the bytes moved per second as a share of HBM peak.  Per-pass times: run it under rocprofv3 --kernel-trace --stats.
usage: python tools/open_rate.py [--log2-n 28] [--cols 20] [--reps 5] [--warmup 1]"""
import argparse
import json
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plonk_gadgets_amd as pg  # noqa: E402
from ntt_rate import FR_MUL_PER_S, HBM_BYTES_PER_S, timed  # noqa: E402

R = pg.transcript.R
RUN = 8  # csrc/opening.hpp: kOpenRun


def fr_mul_count(n, mu):
    """multiplications of one call: pass 1 one per column whose weight is not 1, plus Horner's one; pass 3 per run of RUN points
    RUN - 1 for the run's total, 8 for the lane scan, RUN - 1 for the walk down"""
    muls = sum(1 for m in mu if m % R != 1)
    return n * (muls + 1) + n * (2 * (RUN - 1) + 8) // RUN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=28)
    ap.add_argument("--cols", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    m, n = args.log2_n, 1 << args.log2_n
    eng = pg.Engine(0)
    torch.manual_seed(12)
    cols = []
    for _ in range(args.cols):
        x = torch.randint(0, 2**62, (n, 4), dtype=torch.int64, device="cuda:0")  # (field elements: the top limb < q's)
        cols.append(x)
    rng = random.Random(12)
    x, v2 = rng.randrange(R), rng.randrange(R)
    for name, use, mu in (("xi", cols, [1] + [rng.randrange(R) for _ in range(args.cols - 1)]),
                          ("xi_omega", cols[:4], [1, v2, v2 * v2 % R, pow(v2, 3, R)])):
        out = {}

        def call():
            out["w"] = eng.open(use, mu, x)[0]
        t = timed(call, args.reps, args.warmup)
        sec = t["median"] / 1e3
        muls = fr_mul_count(n, mu)
        moved = (len(use) + 3) * n * 32  # pass 1 reads the columns and writes f; pass 3 reads f and writes the witness
        print(json.dumps({"tool": "open_rate", "aggregate": name, "log2_n": m, "n_cols": len(use), "ms": t,
                          "fr_mul": muls, "fr_mul_per_s": muls / sec, "fr_mul_ceiling_fraction": muls / sec / FR_MUL_PER_S,
                          "bytes": moved, "bytes_per_s": moved / sec, "hbm_fraction": moved / sec / HBM_BYTES_PER_S}), flush=True)
        del out
    eng.close()


if __name__ == "__main__":
    main()
