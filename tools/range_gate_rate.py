"""The three figures of DESIGN section 3.19, one JSON line each (all of them need the GPU):

  --quotient  pg_quotient_range with a live q_range against pg_quotient: the same process, tools/quotient_rate.py's inputs (random
              field elements) plus one more column, the same scratch, calls alternating after the warm-up.  --log2-n 0 takes the
              largest n whose 18 inputs, scratch and output fit the free device memory.  The design's own model (section 3.10)
              expects 76 / 72 transforms and one more pointwise step per chunk: about 1.06.
  --emit      range_gate_batch at 2^20 items of 64 bits (12 rows and 31 Variables an item: 3200 bytes, and one gathered
              assignment): every repetition on a fresh composer, host clock around the call and a synchronise (the call checks its
              Variable array, gathers, and emits); beside it the bare fill of as many bytes in the same process, and the values-only
              refresh after clear_witness.  Bytes per second, and as a share of the 8 TB/s of HBM's specification.
  --prove     one proof of 2^20 items of 64 bits (12 rows each, padded to 2^24): the phases of a proof that reuses the preprocessed
              commitments, the preprocessing, and the same with blinding.
usage: python tools/range_gate_rate.py --quotient|--emit|--prove [--log2-n 0] [--reps 3] [--warmup 1] [--items-log2 20] [--bits 64]"""
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
HBM_PEAK = 8.0e12


def stats(v):
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def timed_once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def witnesses(batch, bits):
    """batch scalars below 2^bits: 4096 pseudo-random ones, repeated (what the emitter stores does not depend on them)"""
    base = torch.from_numpy(synth.uniform_below(min(batch, 1 << 12), 1 << bits, seed=3).view(np.int64)).to("cuda:0")
    return base.repeat((batch + base.shape[0] - 1) // base.shape[0], 1)[:batch].contiguous()


def quotient(args):
    m = args.log2_n
    if m == 0:  # 18 inputs, 8 columns of scratch, 4 of output and one column of slack, 32 bytes a row
        free, _ = torch.cuda.mem_get_info()
        m = min(28, (free // (31 * 32)).bit_length() - 1)
    n = 1 << m
    eng = pg.Engine(0)
    torch.manual_seed(9)
    x = torch.randint(0, 2**62, (18, n, 4), dtype=torch.int64, device="cuda:0")  # (field elements: the top limb < q's)
    polys = {"wires": x[0:4], "z": x[4], "sigmas": x[5:9], "pi": x[16],
             "selectors": {name: x[9 + i] for i, name in enumerate(eng.QUOTIENT_SELECTORS)}}
    scratch = torch.empty((8, n, 4), dtype=torch.int64, device="cuda:0")
    kw = dict(alpha=0x1234_5678 ** 3, beta=0x2345_6789 ** 5, gamma=0x3456_789A ** 7, scratch=scratch)
    calls = {"pg_quotient": lambda: eng.quotient(**polys, **kw), "pg_quotient_range": lambda: eng.quotient(**polys, q_range=x[17], **kw)}
    for _ in range(args.warmup):
        for fn in calls.values():
            timed_once(fn)
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            ms[k].append(timed_once(fn))
    st = {k: stats(v) for k, v in ms.items()}
    out = {"tool": "range_gate_rate --quotient", "log2_n": m, "reps": args.reps, "warmup": args.warmup, "ms": st,
           "range_over_plain": st["pg_quotient_range"]["median"] / st["pg_quotient"]["median"],
           "extra_ms": st["pg_quotient_range"]["median"] - st["pg_quotient"]["median"],
           "transforms": {"pg_quotient": 72, "pg_quotient_range": 76},
           "range_step_bytes": 4 * 7 * n * 32,  # per chunk: a, b, c, a(omega x), q_range and t read, t written
           "expected_about": 1.06}
    print(json.dumps(out), flush=True)
    eng.close()


def emit(args):
    batch, bits = 1 << args.items_log2, args.bits
    k = bits // 2
    g = (k + 2) // 3
    rows, nvars = batch * (g + 1), batch * (k - 1)
    nbytes = rows * 184 + nvars * 32
    eng = pg.Engine(0)
    wit = witnesses(batch, bits)

    def fresh():
        comp = pg.StandardComposer(eng, rows + 16, nvars + batch + 16)
        first = comp.add_input_batch(wit)
        vars_ = torch.arange(first, first + batch, dtype=torch.int64, device="cuda:0")
        comp.sync()
        return comp, vars_
    full, refresh = [], []
    for rep in range(args.warmup + args.reps):
        comp, vars_ = fresh()
        ms = timed_once(lambda: comp.range_gate_batch(vars_, bits))
        assert comp.circuit_size() == 3 + rows
        comp.clear_witness()
        comp.add_input_batch(wit)
        comp.sync()
        ms2 = timed_once(lambda: comp.range_gate_batch(vars_, bits))
        assert comp.refresh_stats() == (rows, 0, True)
        if rep >= args.warmup:
            full.append(ms)
            refresh.append(ms2)
        if rep == args.warmup + args.reps - 1:
            assert comp.check() == -1
        comp.close()
        del comp
        torch.cuda.empty_cache()
    buf = torch.empty((nbytes,), dtype=torch.uint8, device="cuda:0")
    fill = []
    for rep in range(args.warmup + args.reps):
        ms = timed_once(lambda: eng.fill_bytes(buf))
        if rep >= args.warmup:
            fill.append(ms)
    st = {"range_gate_batch": stats(full), "values_only_refresh": stats(refresh), "bare_fill": stats(fill)}
    rate = nbytes / (st["range_gate_batch"]["median"] / 1e3)
    out = {"tool": "range_gate_rate --emit", "items": batch, "num_bits": bits, "rows_per_item": g + 1, "vars_per_item": k - 1,
           "bytes": nbytes, "reps": args.reps, "warmup": args.warmup, "ms": st, "bytes_per_s": rate,
           "of_hbm_peak_8TBps": rate / HBM_PEAK, "of_bare_fill": st["bare_fill"]["median"] / st["range_gate_batch"]["median"],
           "refresh_bytes": nvars * 32, "refresh_bytes_per_s": nvars * 32 / (st["values_only_refresh"]["median"] / 1e3),
           "note": "the call's time holds the device check of the Variable array (a host synchronisation) and the gather of the assignments"}
    print(json.dumps(out), flush=True)
    eng.close()


def prove(args):
    batch, bits = 1 << args.items_log2, args.bits
    k = bits // 2
    g = (k + 2) // 3
    rows, nvars = batch * (g + 1), batch * (k - 1)
    eng = pg.Engine(0)
    wit = witnesses(batch, bits)
    comp = pg.StandardComposer(eng, rows + 16, nvars + batch + 16)
    first = comp.add_input_batch(wit)
    comp.range_gate_batch(torch.arange(first, first + batch, dtype=torch.int64, device="cuda:0"), bits)
    comp.sync()
    n = 1 << (comp.circuit_size() - 1).bit_length()
    assert comp.check() == -1
    t = time.perf_counter()
    ck = pg.CommitKey.setup(eng, n - 1 + 8, S(0x5EED_7A0 ** 9))
    torch.cuda.synchronize()
    setup_ms = (time.perf_counter() - t) * 1e3
    ok = pg.OpeningKey.setup(eng, S(0x5EED_7A0 ** 9))
    t = time.perf_counter()
    pre = comp.preprocessed_commitments(ck)
    torch.cuda.synchronize()
    pre_ms = (time.perf_counter() - t) * 1e3
    out = {"tool": "range_gate_rate --prove", "items": batch, "num_bits": bits, "rows": comp.circuit_size(), "log2_n": n.bit_length() - 1,
           "srs_setup_ms": setup_ms, "preprocess_ms": pre_ms}
    vk = pg.VerifierKey(n, pre)
    for name, blinding in (("plain", None), ("blinded", True)):
        comp.prove(ck, b"plonk", pre, blinding=blinding)  # warm-up
        phases = {}
        t = time.perf_counter()
        proof = comp.prove(ck, b"plonk", pre, timings=phases, blinding=blinding)
        ms = (time.perf_counter() - t) * 1e3
        assert proof.verify(vk, ok, {})
        out[name] = {"prove_ms": ms, "phases_ms": phases, "msm_ms": sum(v for k_, v in phases.items() if k_.endswith("_msm"))}
    print(json.dumps(out), flush=True)
    comp.close()
    ok.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quotient", action="store_true")
    ap.add_argument("--emit", action="store_true")
    ap.add_argument("--prove", action="store_true")
    ap.add_argument("--log2-n", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--items-log2", type=int, default=20)
    ap.add_argument("--bits", type=int, default=64)
    args = ap.parse_args()
    if args.quotient:
        quotient(args)
    if args.emit:
        emit(args)
    if args.prove:
        prove(args)


if __name__ == "__main__":
    main()
