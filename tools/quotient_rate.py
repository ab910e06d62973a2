"""Times pg_quotient (csrc/quotient.hpp) at 2^28 on random inputs, warmed up, and in the same process the 72 n-point transforms
it runs (17 x 4 coset-forward, 4 coset-inverse) timed alone through pg_ntt.  One JSON line: per call median / min / max ms, the
transforms' ms, the share of the call outside them (pointwise steps, combine, tables), the field multiplications per second and
their share of the fr_mul ceiling (tools/fr_mul_bench.hip), and the ratio the design targets (call / transforms <= 1.15).
usage: python tools/quotient_rate.py [--log2-n 28] [--reps 3] [--warmup 1]

With --blinded it times pg_quotient_blinded against pg_quotient instead: the same process, the same inputs
(the blinded call reads two more rows of each wire and three of z, random like the rest), the same scratch, calls alternating after
the warm-up; one JSON line with both calls' ms and their ratio (the design expects <= 1.04).  --log2-n 0 then takes the largest
n whose 17 inputs, scratch and output fit the free device memory.
usage: python tools/quotient_rate.py --blinded [--log2-n 0] [--reps 3] [--warmup 1]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plonk_gadgets_amd as pg  # noqa: E402
from ntt_rate import FR_MUL_PER_S, counts, timed  # noqa: E402

# multiplications per point of a chunk in the pointwise steps (csrc/quotient.hpp): QS_PERM_NUM 18 (x and n x twice, the trick's
# three, beta k_j x four, the product four, alpha, L1 two), QS_GATE1 3, QS_GATE2 2, QS_GATE3 1, QS_PERM1 3, QS_PERM2 7; the
# combine 5 per k0
POINTWISE_FR_MUL_PER_POINT = 18 + 3 + 2 + 1 + 3 + 7
COMBINE_FR_MUL = 5


def blinded(args):
    import numpy as np
    m = args.log2_n
    if m == 0:  # 17 inputs, 8 columns of scratch, 4 of output and one column of slack, 32 bytes a row
        free, _ = torch.cuda.mem_get_info()
        m = min(28, (free // (30 * 32)).bit_length() - 1)
    n = 1 << m
    eng = pg.Engine(0)
    torch.manual_seed(9)
    x = torch.randint(0, 2**62, (17, n + 4, 4), dtype=torch.int64, device="cuda:0")  # (field elements: the top limb < q's)
    rest = {"sigmas": [x[5 + j, :n] for j in range(4)], "pi": x[16, :n],
            "selectors": {name: x[9 + i, :n] for i, name in enumerate(eng.QUOTIENT_SELECTORS)}}
    scratch = torch.empty((8, n, 4), dtype=torch.int64, device="cuda:0")
    kw = dict(alpha=0x1234_5678 ** 3, beta=0x2345_6789 ** 5, gamma=0x3456_789A ** 7, scratch=scratch)
    plain = lambda: eng.quotient([x[j, :n] for j in range(4)], x[4, :n], **rest, **kw)
    blind = lambda: eng.quotient_blinded([x[j, :n + 2] for j in range(4)], x[4, :n + 3], **rest, **kw)

    def once(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()  # (both calls only enqueue)
        ms = (time.perf_counter() - t) * 1e3
        torch.cuda.empty_cache()  # (the two outputs differ by eight rows: neither keeps the other's block)
        return ms
    for _ in range(args.warmup):
        once(plain), once(blind)
    ms = {"pg_quotient": [], "pg_quotient_blinded": []}
    for _ in range(args.reps):
        ms["pg_quotient"].append(once(plain))
        ms["pg_quotient_blinded"].append(once(blind))
    stat = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in ms.items()}
    out = {"tool": "quotient_rate --blinded", "log2_n": m, "reps": args.reps, "warmup": args.warmup, "ms": stat,
           "blinded_over_plain": stat["pg_quotient_blinded"]["median"] / stat["pg_quotient"]["median"],
           "extra_ms": stat["pg_quotient_blinded"]["median"] - stat["pg_quotient"]["median"],
           "blind_step_bytes": 4 * 10 * n * 32, "expected_at_most": 1.04}
    print(json.dumps(out), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--blinded", action="store_true", help="time pg_quotient_blinded against pg_quotient (see the module's text)")
    args = ap.parse_args()
    if args.blinded:
        return blinded(args)
    m, n = args.log2_n, 1 << args.log2_n
    eng = pg.Engine(0)
    torch.manual_seed(9)
    x = torch.randint(0, 2**62, (17, n, 4), dtype=torch.int64, device="cuda:0")  # (field elements: the top limb < q's)
    polys = {"wires": x[0:4], "z": x[4], "sigmas": x[5:9], "pi": x[16],
             "selectors": {name: x[9 + i] for i, name in enumerate(eng.QUOTIENT_SELECTORS)}}
    scratch = torch.empty((8, n, 4), dtype=torch.int64, device="cuda:0")
    kw = dict(alpha=0x1234_5678 ** 3, beta=0x2345_6789 ** 5, gamma=0x3456_789A ** 7, scratch=scratch)
    call = timed(lambda: eng.quotient(**polys, **kw), args.reps, args.warmup)
    zeta, g = pg.domain_generator(m + 2).to_int(), pg.DEFAULT_COSET_GENERATOR
    q = pg.scalar.Q

    def transforms():
        for j in range(4):
            gj = g * pow(zeta, j, q) % q
            for i in range(17):
                eng.coset_fft(scratch[i % 8], g=gj, inplace=True)
            eng.coset_ifft(scratch[j], g=gj, inplace=True)
    alone = timed(transforms, args.reps, args.warmup)
    mul_t = 68 * counts(m, "coset_fft")["fr_mul"] + 4 * counts(m, "coset_ifft")["fr_mul"]
    mul_p = 4 * n * POINTWISE_FR_MUL_PER_POINT + n * COMBINE_FR_MUL
    sec = call["median"] / 1e3
    out = {"tool": "quotient_rate", "log2_n": m, "ms": call, "transforms_alone_ms": alone, "transforms": 72,
           "call_over_transforms": call["median"] / alone["median"],
           "pointwise_share": 1 - alone["median"] / call["median"],
           "fr_mul": mul_t + mul_p, "fr_mul_transforms": mul_t, "fr_mul_pointwise": mul_p,
           "fr_mul_per_s": (mul_t + mul_p) / sec, "fr_mul_ceiling_fraction": (mul_t + mul_p) / sec / FR_MUL_PER_S,
           "hbm_gib": {"inputs": 17 * n * 32 / 2**30, "t": 4 * n * 32 / 2**30, "scratch": 8 * n * 32 / 2**30}}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
