"""Times pg_sigma_evaluations and pg_permutation_product (csrc/permutation_product.hpp) on bench.py's next_rows composer (built as bench.next_rows_secondary builds it):
2^18 x (allocate + range_check(0, 2^254)) = 270 270 467 rows, padded to 2^29.  One JSON line: per call median / min / max ms,
rows/s, field multiplications/s and their share of the fr_mul ceiling (tools/fr_mul_bench.hip), and the HBM share of the
algorithmic bytes.
usage: python tools/perm_product_rate.py [--log2-batch 18] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import plonk_gadgets_amd as pg  # noqa: E402
from plonk_gadgets_amd import synth  # noqa: E402

FR_MUL_PER_S = 1.32e11   # tools/fr_mul_bench.hip on MI355X
HBM_BYTES_PER_S = 8.0e12  # MI355X peak
# multiplications per row: 8 table products, 6 to combine the factors, 5 for the batch inversion and the
# tile products (Montgomery's trick: 4, lane product 1), 2 for the scan (the lanes' products and the running product); the
# inversions (one per 64 rows) and the scans of the lanes' and tiles' products are left out
MULS_PER_ROW_PRODUCT = 21
# bytes per row the algorithm must move: four wire values (32 B), four sigma entries (8 B), z (32 B)
BYTES_PER_ROW_PRODUCT = 4 * 32 + 4 * 8 + 32
# per sigma entry: the entry (8 B) and its evaluation (32 B); one multiplication
BYTES_PER_ENTRY_EVAL = 8 + 32


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()  # (both calls synchronise their stream before they return)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-batch", type=int, default=18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    eng = pg.Engine(0)
    S = pg.BlsScalar.from_int
    batch = 1 << args.log2_batch
    comp = pg.StandardComposer(eng, 3 + batch * 1031 + 8, 5 + batch * 1034 + 8)
    wit = torch.from_numpy(synth.random_scalars(batch, seed=synth.SEED + 2).view(np.int64)).to("cuda:0")
    comp.range_check_batch(S(0), S(2**254), wit)
    n = comp.circuit_size()
    padded_n = 1 << (n - 1).bit_length()
    sigma = comp.permutation(padded_n)
    vals = comp.wire_values()
    beta, gamma = S(0x5EED_0001 ** 9), S(0x5EED_0002 ** 11)
    out = {"tool": "perm_product_rate", "rows": n, "padded_n": padded_n}
    z_wrap = []

    def product():
        z_wrap[:] = eng.permutation_product(vals, sigma, beta, gamma)
    t = timed(product, args.reps, args.warmup)
    assert z_wrap[1].to_int() == 1
    sec = t["median"] / 1e3
    out["permutation_product"] = {
        "ms": t, "rows_per_s": padded_n / sec,
        "fr_mul_per_s": MULS_PER_ROW_PRODUCT * padded_n / sec,
        "fr_mul_ceiling_fraction": MULS_PER_ROW_PRODUCT * padded_n / sec / FR_MUL_PER_S,
        "hbm_fraction_of_algorithmic_bytes": BYTES_PER_ROW_PRODUCT * padded_n / sec / HBM_BYTES_PER_S,
        "muls_per_row_counted": MULS_PER_ROW_PRODUCT, "algorithmic_bytes": BYTES_PER_ROW_PRODUCT * padded_n,
        "kernels": "pp_tables_kernel + pp_ratio_kernel + pp_carry_kernel + pp_scan_kernel"}
    del z_wrap[:], vals
    torch.cuda.empty_cache()
    ev = []

    def evaluations():
        ev[:] = [eng.sigma_evaluations(sigma)]
    t = timed(evaluations, args.reps, args.warmup)
    sec = t["median"] / 1e3
    out["sigma_evaluations"] = {
        "ms": t, "entries_per_s": 4 * padded_n / sec,
        "fr_mul_per_s": 4 * padded_n / sec, "fr_mul_ceiling_fraction": 4 * padded_n / sec / FR_MUL_PER_S,
        "hbm_fraction_of_algorithmic_bytes": BYTES_PER_ENTRY_EVAL * 4 * padded_n / sec / HBM_BYTES_PER_S,
        "algorithmic_bytes": BYTES_PER_ENTRY_EVAL * 4 * padded_n, "kernels": "pp_tables_kernel + pp_sigma_eval_kernel"}
    print(json.dumps(out), flush=True)
    comp.close()
    eng.close()


if __name__ == "__main__":
    main()
