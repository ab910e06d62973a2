"""Times pg_msm (csrc/msm.hpp) at 2^28 on an SRS from pg_srs_setup and random scalars, warmed up: a single-column call, a
4-column call, and pg_srs_setup itself at the same size.  One JSON line: per call median / min / max ms, and the bucket
accumulation's field multiplications per second (n mixed additions per window at 10 Fq multiplications each, 16 windows) as a
share of the fq_mul ceiling (tools/fq_mul_bench.hip; pass --fq-mul-per-s with the figure measured on the box).
usage: python tools/msm_rate.py [--log2-n 28] [--reps 3] [--warmup 1] [--fq-mul-per-s 5e10]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plonk_gadgets_amd as pg  # noqa: E402
from ntt_rate import timed  # noqa: E402

FQ_MUL_PER_MADD = 10  # madd-2008-s: 8 multiplications + 2 squarings
WINDOWS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fq-mul-per-s", type=float, default=5e10)
    args = ap.parse_args()
    m, n = args.log2_n, 1 << args.log2_n
    eng = pg.Engine(0)
    tau = pg.BlsScalar.from_int(0x5EED_7A0 ** 9)
    holder = {}

    def setup():
        holder.pop("ck", None)
        holder["ck"] = pg.CommitKey.setup(eng, n - 1, tau)
    srs = timed(setup, 1, 0)
    ck = holder["ck"]
    g = torch.Generator(device="cuda:0").manual_seed(28)
    x = torch.randint(0, 2**62, (4, n, 4), dtype=torch.int64, device="cuda:0", generator=g)
    one = timed(lambda: ck.commit(x[0]), args.reps, args.warmup)
    four = timed(lambda: ck.commit(x), args.reps, args.warmup)
    madd = WINDOWS * n * FQ_MUL_PER_MADD
    out = {"tool": "msm_rate", "log2_n": m, "msm_1col_ms": one, "msm_4col_ms": four, "srs_setup_ms": srs,
           "bucket_fq_mul": madd, "bucket_fq_mul_per_s": madd / (one["median"] / 1e3),
           "fq_mul_ceiling_per_s": args.fq_mul_per_s,
           "bucket_fq_mul_ceiling_fraction": madd / (one["median"] / 1e3) / args.fq_mul_per_s,
           "target_1col_ms": 2500, "hbm_gib": {"srs": n * 96 / 2**30, "scalars": 4 * n * 32 / 2**30}}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
