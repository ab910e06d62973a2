"""The figures of DESIGN section 3.20 (all of them need the GPU); each mode prints one JSON line and stores it under its own key in
--out (default profiles/interval_gate_rate.json):

  --emit      interval_gate at 2^20 items of 64 bits (24 rows and 64 Variables an item: 6464 bytes, and one gathered assignment),
              with one pair of bounds for the call and with a pair per item: every repetition on a fresh composer, host clock
              around the call and a synchronise (the call checks its arrays, gathers, and emits), and the values-only refresh after
              clear_witness.  In the same process, alternating with them, the same statement assembled from older calls on uniform
              bounds -- two add_batch calls for the differences, then two range_gate_batch calls (26 rows and 64 Variables an item)
              -- and the bare fill of the fused call's bytes.
  --kernels F the emitter ALONE: --emit was run under `rocprofv3 --kernel-trace` and F is the trace that run left (its database, or
              a kernel-trace CSV); the durations of each IntervalGateGD emitter and of the calls' other kernels are stored beside --emit's
              figures (the host clock of --emit holds a host synchronisation and the gather; the trace does not).
  --prove     the headline, proven: 2^items-log2 items of interval_gate(w, min_i, max_i, 64) with a pair per item (2^20: 25 165 824
              rows, padded to 2^25): check(), the preprocessing, and the phases of a proof that reuses the preprocessed commitments,
              unblinded and blinded; Proof.verify accepts both.
usage: python tools/interval_gate_rate.py --emit|--prove|--kernels F [--reps 3] [--warmup 1] [--items-log2 20] [--bits 64] [--out F]"""
import argparse
import csv
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
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
DEV = "cuda:0"


def stats(v):
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def timed_once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def store(args, key, out):
    print(json.dumps(out), flush=True)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc[key] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def repeated(base, batch):
    return base.repeat((batch + base.shape[0] - 1) // base.shape[0], 1)[:batch].contiguous()


def inputs(batch, bits):
    """(witnesses, per-item min, per-item max) on the device: 4096 pseudo-random triples with min <= witness <= max and
    max - min < 2^bits, repeated (what the emitter stores does not depend on them); the uniform pair [LO, LO + 2^bits) holds every
    witness too"""
    m = min(batch, 1 << 12)
    rnd = np.random.default_rng(3)
    off = [int(x) for x in rnd.integers(0, 1 << (bits - 1), m)]
    below = [int(x) for x in rnd.integers(0, 1 << (bits - 2), m)]
    above = [int(x) for x in rnd.integers(0, 1 << (bits - 2), m)]
    lo0 = 10**6
    wit = [lo0 + (1 << (bits - 2)) + o for o in off]
    to_dev = lambda xs: repeated(torch.from_numpy(synth.scalars_from_ints(xs).view(np.int64)).to(DEV), batch)
    return to_dev(wit), to_dev([w - b for w, b in zip(wit, below)]), to_dev([w + a for w, a in zip(wit, above)]), (lo0, lo0 + (1 << bits) - 1)


def shape(bits):
    k = bits // 2
    g = (k + 2) // 3
    return k, g


def emit(args):
    batch, bits = 1 << args.items_log2, args.bits
    k, g = shape(bits)
    rows, nvars = batch * 2 * (g + 1), batch * 2 * k
    nbytes = rows * 184 + nvars * 32
    eng = pg.Engine(0)
    wit, lo_v, hi_v, (lo, hi) = inputs(batch, bits)

    def fresh():
        comp = pg.StandardComposer(eng, rows + 2 * batch + 16, nvars + batch + 16)
        first = comp.add_input_batch(wit)
        vars_ = torch.arange(first, first + batch, dtype=torch.int64, device=DEV)
        comp.sync()
        return comp, vars_

    def assembled(comp, v):
        d_lo = comp.add_batch(S(1), v, S(0), v, S(R - lo))      # w - min
        d_hi = comp.add_batch(S(R - 1), v, S(0), v, S(hi))      # max - w
        comp.range_gate_batch(d_lo, bits)
        comp.range_gate_batch(d_hi, bits)
    forms = {"interval_gate_batch": lambda comp, v: comp.interval_gate_batch(v, S(lo), S(hi), bits),
             "interval_gate_ragged_batch": lambda comp, v: comp.interval_gate_ragged_batch(v, lo_v, hi_v, bits),
             "assembled_add_batch_x2_range_gate_batch_x2": assembled}
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    ms = {name: [] for name in forms}
    ms.update({name + "_refresh": [] for name in forms})
    ms["bare_fill"] = []
    refreshed = {}
    for rep in range(args.warmup + args.reps):
        order = list(forms) if rep % 2 == 0 else list(forms)[::-1]  # alternating order
        for name in order:
            comp, vars_ = fresh()
            t_full = timed_once(lambda: forms[name](comp, vars_))
            n_rows = comp.circuit_size() - 3
            assert n_rows == (rows if name.startswith("interval") else rows + 2 * batch), (name, n_rows)
            comp.clear_witness()
            comp.add_input_batch(wit)
            comp.sync()
            t_ref = timed_once(lambda: forms[name](comp, vars_))
            refreshed[name] = comp.refresh_stats()
            assert not name.startswith("interval") or refreshed[name] == (n_rows, 0, True), (name, refreshed[name])
            if rep == args.warmup + args.reps - 1:
                assert comp.check() == -1, name
            comp.close()
            del comp
            torch.cuda.empty_cache()
            t_fill = timed_once(lambda: eng.fill_bytes(buf))
            if rep >= args.warmup:
                ms[name].append(t_full)
                ms[name + "_refresh"].append(t_ref)
                ms["bare_fill"].append(t_fill)
    st = {name: stats(v) for name, v in ms.items()}
    fused, asm = st["interval_gate_batch"]["median"], st["assembled_add_batch_x2_range_gate_batch_x2"]["median"]
    out = {"tool": "interval_gate_rate --emit", "items": batch, "num_bits": bits, "rows_per_item": 2 * (g + 1), "vars_per_item": 2 * k,
           "bytes": nbytes, "assembled_bytes": nbytes + 2 * batch * 184, "reps": args.reps, "warmup": args.warmup, "ms": st,
           "bytes_per_s": nbytes / (fused / 1e3), "of_hbm_peak_8TBps": nbytes / (fused / 1e3) / HBM_PEAK,
           "of_bare_fill": st["bare_fill"]["median"] / fused,
           "per_item_bytes_per_s": nbytes / (st["interval_gate_ragged_batch"]["median"] / 1e3),
           "assembled_over_fused": asm / fused,
           "refresh_stats": {name: list(v) for name, v in refreshed.items()},
           "refresh_bytes": nvars * 32, "refresh_bytes_per_s": nvars * 32 / (st["interval_gate_batch_refresh"]["median"] / 1e3),
           "note": "a call's time holds the device check of its arrays (one host synchronisation per call: four in the assembled form) "
                   "and the gather of the assignments; --kernels has the emitter alone"}
    store(args, "emit", out)
    eng.close()


KERNELS_OF_THE_CALLS = ("IntervalGateGD", "RangeGateGD", "interval_bounds_kernel", "max_variable_kernel", "gather_wire_values_kernel",
                        "fill_kernel", "gate_batch")


def kernels(args):
    """per kernel of the calls --emit makes: dispatches and their durations in microseconds, from the trace a run of --emit under
    rocprofv3 --kernel-trace left (its rocpd database, or a kernel-trace CSV with Kernel_Name, Start_Timestamp, End_Timestamp)"""
    durations = {}
    if args.kernels.endswith(".db"):
        import sqlite3
        with sqlite3.connect(args.kernels) as db:
            for name, ns in db.execute("select name, duration from kernels"):
                durations.setdefault(name, []).append(ns / 1e3)
    else:
        with open(args.kernels) as f:
            for r in csv.DictReader(f):
                durations.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = [{"kernel": name, "calls": len(v), "median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)}
            for name, v in sorted(durations.items()) if any(s in name for s in KERNELS_OF_THE_CALLS)]
    store(args, "kernels", {"tool": "interval_gate_rate --kernels", "source": "rocprofv3 --kernel-trace around --emit --reps 3 --warmup 1",
                            "kernels": rows})


def prove(args):
    batch, bits = 1 << args.items_log2, args.bits
    k, g = shape(bits)
    rows, nvars = batch * 2 * (g + 1), batch * 2 * k
    eng = pg.Engine(0)
    wit, lo_v, hi_v, _ = inputs(batch, bits)
    comp = pg.StandardComposer(eng, rows + 16, nvars + batch + 16)
    first = comp.add_input_batch(wit)
    comp.interval_gate_ragged_batch(torch.arange(first, first + batch, dtype=torch.int64, device=DEV), lo_v, hi_v, bits)
    comp.sync()
    del wit, lo_v, hi_v
    n = 1 << (comp.circuit_size() - 1).bit_length()
    out = {"tool": "interval_gate_rate --prove", "items": batch, "num_bits": bits, "rows": comp.circuit_size(), "log2_n": n.bit_length() - 1}
    check_ms = timed_once(lambda: out.__setitem__("check", comp.check()))
    assert out["check"] == -1
    out["check_ms"] = check_ms
    t = time.perf_counter()
    ck = pg.CommitKey.setup(eng, n - 1 + 8, S(0x5EED_7A0 ** 9))
    torch.cuda.synchronize()
    out["srs_setup_ms"] = (time.perf_counter() - t) * 1e3
    ok = pg.OpeningKey.setup(eng, S(0x5EED_7A0 ** 9))
    t = time.perf_counter()
    pre = comp.preprocessed_commitments(ck)
    torch.cuda.synchronize()
    out["preprocess_ms"] = (time.perf_counter() - t) * 1e3
    vk = pg.VerifierKey(n, pre)
    for name, blinding in (("plain", None), ("blinded", True)):
        if args.warmup:
            comp.prove(ck, b"plonk", pre, blinding=blinding)
        phases = {}
        t = time.perf_counter()
        proof = comp.prove(ck, b"plonk", pre, timings=phases, blinding=blinding)
        ms = (time.perf_counter() - t) * 1e3
        assert proof.verify(vk, ok, {})
        out[name] = {"prove_ms": ms, "verified": True, "phases_ms": phases,
                     "msm_ms": sum(v for k_, v in phases.items() if k_.endswith("_msm"))}
        store(args, "prove", out)  # (kept as far as it got, should the next proof not fit)
    comp.close()
    ok.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emit", action="store_true")
    ap.add_argument("--prove", action="store_true")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--items-log2", type=int, default=20)
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "interval_gate_rate.json"))
    args = ap.parse_args()
    if args.emit:
        emit(args)
    if args.kernels:
        kernels(args)
    if args.prove:
        prove(args)


if __name__ == "__main__":
    main()
