"""Times pg_ntt (csrc/ntt.hpp) at 2^29 points, warmed up: a forward and an inverse transform of one random column, and an inverse
transform of four columns in one call.  One JSON line: per call median / min / max ms, the field multiplications the kernels do per
second and their share of the fr_mul ceiling (tools/fr_mul_bench.hip), and the HBM share of the bytes the passes move.
usage: python tools/ntt_rate.py [--log2-n 29] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import plonk_gadgets_amd as pg  # noqa: E402

FR_MUL_PER_S = 1.32e11   # tools/fr_mul_bench.hip on MI355X
HBM_BYTES_PER_S = 8.0e12  # MI355X peak
TILE_BITS, STRIDED_BITS = 10, 7  # csrc/ntt.hpp: kNttTileBits, kNttStridedBits


def plan(m: int) -> list:
    """the points per column (log2) of each pass, as pg_ntt splits them"""
    if m <= TILE_BITS:
        return [m]
    top = m - TILE_BITS
    np_ = (top + STRIDED_BITS - 1) // STRIDED_BITS
    return [top // np_ + (1 if p < top % np_ else 0) for p in range(np_)] + [TILE_BITS]


def counts(m: int, kind: str) -> dict:
    """multiplications and bytes of one column: radix-2 butterflies (the last stage of a pass has none), two per point for
    each twiddle (table lookup and product), two per point for a coset scaling, one for ifft's n^-1"""
    n, ks = 1 << m, plan(m)
    muls = sum(n // 2 * (k - 1) for k in ks if k) + 2 * n * (len(ks) - 1)
    muls += {"fft": 0, "ifft": n, "coset_fft": 2 * n, "coset_ifft": 2 * n}[kind]
    memory_passes = len(ks) + (1 if m > TILE_BITS else 0)  # (+ the bit-reversal pass)
    return {"fr_mul": muls, "bytes": memory_passes * 2 * 32 * n, "passes": ks, "memory_passes": memory_passes,
            "butterfly_bound_fr_mul": n // 2 * m}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()  # (pg_ntt only enqueues)
        ms.append((time.perf_counter() - t) * 1e3)
    return {"median": float(np.median(ms)), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=29)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    m, n = args.log2_n, 1 << args.log2_n
    eng = pg.Engine(0)
    torch.manual_seed(8)
    out = {"tool": "ntt_rate", "log2_n": m}
    for name, cols, kind in (("fft_1col", 1, "fft"), ("ifft_1col", 1, "ifft"), ("ifft_4col", 4, "ifft")):
        x = torch.randint(0, 2**62, (cols, n, 4), dtype=torch.int64, device="cuda:0")  # (field elements: the top limb < q's)
        fn = getattr(eng, kind)
        t = timed(lambda: fn(x, inplace=True), args.reps, args.warmup)
        c = counts(m, kind)
        sec = t["median"] / 1e3
        out[name] = {"ms": t, "ms_per_column": t["median"] / cols, "columns": cols,
                     "fr_mul_per_s": cols * c["fr_mul"] / sec, "fr_mul_ceiling_fraction": cols * c["fr_mul"] / sec / FR_MUL_PER_S,
                     "hbm_fraction": cols * c["bytes"] / sec / HBM_BYTES_PER_S, "fr_mul_per_column": c["fr_mul"],
                     "bytes_per_column": c["bytes"], "pass_bits": c["passes"], "memory_passes": c["memory_passes"],
                     "butterfly_bound_fr_mul_per_column": c["butterfly_bound_fr_mul"]}
        del x
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
