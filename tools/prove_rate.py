"""Times StandardComposer.prove on padded range_check composers (batches of allocate + range_check(0, 2^254), 1031 rows each) at
2^22, 2^24 and 2^26 rows: one JSON line per size with the phase times of tools' first proof (preprocessing included) and of a
second proof that reuses the preprocessed commitments, each round's MSMs, the quotient, the evaluations and round 5's device work
(the two openings), and the MSMs' share of a proof.  The device is synchronised between phases, so the phases add up to the
proof.  With --blinded each line also carries a blinded proof of the same circuit (prove(..., blinding=True) under a key of eight
more powers, after one blinded proof to warm up): its phases, and blinded / unblinded per phase and in all.
usage: python tools/prove_rate.py [--log2-n 22 24 26] [--blinded]"""
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

S = pg.BlsScalar.from_int
ROWS_PER_ITEM = 1031


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, nargs="+", default=[22, 24, 26])
    ap.add_argument("--blinded", action="store_true", help="also time a blinded proof of each circuit")
    args = ap.parse_args()
    eng = pg.Engine(0)
    top = max(args.log2_n)
    extra = 8 if args.blinded else 0  # a blinded proof commits to t_4 of n + 8 coefficients
    t = time.perf_counter()
    ck_all = pg.CommitKey.setup(eng, (1 << top) - 1 + extra, S(0x5EED_7A0 ** 9))
    torch.cuda.synchronize()
    setup_ms = (time.perf_counter() - t) * 1e3
    for m in args.log2_n:
        n = 1 << m
        batch = (n - 16) // ROWS_PER_ITEM
        comp = pg.StandardComposer(eng, batch * ROWS_PER_ITEM + 16, batch * 1034 + 16)
        w = torch.from_numpy(synth.random_scalars(batch, seed=m).view(np.int64)).to("cuda:0")
        comp.range_check_batch(S(0), S(2**254), w)
        comp.sync()
        assert 1 << (comp.circuit_size() - 1).bit_length() == n
        ck = ck_all.trim(n - 1)
        first, second = {}, {}
        t = time.perf_counter()
        pre = comp.preprocessed_commitments(ck)
        torch.cuda.synchronize()
        first["preprocess"] = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        p1 = comp.prove(ck, b"plonk", pre, timings=first)
        first_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        p2 = comp.prove(ck, b"plonk", pre, timings=second)
        second_ms = (time.perf_counter() - t) * 1e3
        assert p1.to_bytes() == p2.to_bytes()
        msm = sum(v for k, v in second.items() if k.endswith("_msm"))
        out = {"tool": "prove_rate", "log2_n": m, "rows": comp.circuit_size(), "srs_setup_ms": setup_ms,
               "preprocess_ms": first["preprocess"], "prove_ms": second_ms, "prove_first_ms": first_ms,
               "phases_ms": second, "msm_ms": msm, "msm_share": msm / second_ms,
               "round5_device_share": second.get("round5_open", 0.0) / second_ms}
        if args.blinded:
            ckb, phases = ck_all.trim(n - 1 + extra), {}
            comp.prove(ckb, b"plonk", pre, blinding=True)
            t = time.perf_counter()
            pb = comp.prove(ckb, b"plonk", pre, timings=phases, blinding=True)
            blinded_ms = (time.perf_counter() - t) * 1e3
            assert pb.to_bytes() != p2.to_bytes()
            out.update({"blinded_prove_ms": blinded_ms, "blinded_phases_ms": phases, "blinded_over_plain": blinded_ms / second_ms,
                        "blinded_over_plain_phases": {k: phases[k] / second[k] for k in second}})
            del ckb
        print(json.dumps(out), flush=True)
        comp.close()
        del pre, ck, w
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
