"""The figures of DESIGN section 3.23 (they need the GPU); each mode prints one JSON line and stores it under its own key in --out
(default profiles/compare_gate_rate.json):

  --emit      is_less_equal_each at 2^20 items of 64 bits (12 rows and 33 Variables an item: 3264 bytes, and two gathered
              assignments): every repetition on a fresh composer, host clock around the call and a synchronise (the call checks its
              arrays, gathers, and emits), and the values-only refresh after clear_witness.  In the same process, alternating with
              it, the same rows assembled from calls that existed before the gadget -- add_batch(-1 x + 1 y + 2^64), then
              range_gate_batch(z, 66): 13 rows and 33 Variables an item -- and the bare fill of the fused call's bytes.
  --kernels F the kernels ALONE: --emit was run under `rocprofv3 --kernel-trace` and F is the trace that run left (its database, or
              a kernel-trace CSV); the durations of the CompareGateGD emitters and of the calls' other kernels are stored beside
              --emit's figures (the host clock of --emit holds a host synchronisation and the gathers; the trace does not).
usage: python tools/compare_gate_rate.py --emit|--kernels F [--reps 5] [--warmup 1] [--items-log2 20] [--bits 64] [--out F]"""
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


def inputs(batch, bits):
    """2 * batch scalars on the device, x then y: 4096 pseudo-random pairs below 2^bits, a third of them with x > y, a third equal,
    repeated (what the emitter stores does not depend on them)"""
    m = min(batch, 1 << 12)
    rnd = np.random.default_rng(3)
    a = [int(v) for v in rnd.integers(0, 1 << (bits - 1), m)]
    b = [int(v) for v in rnd.integers(0, 1 << (bits - 1), m)]
    xs = [max(p, q) if i % 3 == 0 else min(p, q) for i, (p, q) in enumerate(zip(a, b))]
    ys = [min(p, q) if i % 3 == 0 else (x if i % 3 == 1 else max(p, q)) for i, (p, q, x) in enumerate(zip(a, b, xs))]

    def to_dev(vals):
        base = torch.from_numpy(synth.scalars_from_ints(vals).view(np.int64)).to(DEV)
        return base.repeat((batch + m - 1) // m, 1)[:batch]
    return torch.cat([to_dev(xs), to_dev(ys)]).contiguous()


def emit(args):
    batch, bits = 1 << args.items_log2, args.bits
    k = bits // 2 + 1
    g = (k + 2) // 3
    rows, nvars = batch * (g + 1), batch * k
    nbytes = rows * 184 + nvars * 32
    eng = pg.Engine(0)
    wit = inputs(batch, bits)

    def fresh():
        comp = pg.StandardComposer(eng, rows + batch + 16, nvars + 2 * batch + 16)
        first = comp.add_input_batch(wit)
        xs = torch.arange(first, first + batch, dtype=torch.int64, device=DEV)
        comp.sync()
        return comp, xs, xs + batch

    def assembled(comp, xs, ys):
        z = comp.add_batch(S(-1 % synth.Q), xs, S(1), ys, S(1 << bits))      # 2^bits + y - x
        comp.range_gate_batch(z, bits + 2)
    forms = {"is_less_equal_each": lambda comp, xs, ys: comp.is_less_equal_each(xs, ys, bits),
             "assembled_add_batch_range_gate_batch": assembled}
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    ms = {name: [] for name in forms}
    ms.update({name + "_refresh": [] for name in forms})
    ms["bare_fill"] = []
    refreshed = {}
    for rep in range(args.warmup + args.reps):
        order = list(forms) if rep % 2 == 0 else list(forms)[::-1]  # alternating order
        for name in order:
            comp, xs, ys = fresh()
            t_full = timed_once(lambda: forms[name](comp, xs, ys))
            n_rows = comp.circuit_size() - 3
            assert n_rows == (rows if name == "is_less_equal_each" else rows + batch), (name, n_rows)
            comp.clear_witness()
            comp.add_input_batch(wit)
            comp.sync()
            t_ref = timed_once(lambda: forms[name](comp, xs, ys))
            refreshed[name] = comp.refresh_stats()
            assert name != "is_less_equal_each" or refreshed[name] == (n_rows, 0, True), (name, refreshed[name])
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
    fused, asm = st["is_less_equal_each"]["median"], st["assembled_add_batch_range_gate_batch"]["median"]
    out = {"tool": "compare_gate_rate --emit", "items": batch, "num_bits": bits, "rows_per_item": g + 1, "vars_per_item": k,
           "bytes": nbytes, "assembled_bytes": nbytes + batch * 184, "reps": args.reps, "warmup": args.warmup, "ms": st,
           "bytes_per_s": nbytes / (fused / 1e3), "of_hbm_peak_8TBps": nbytes / (fused / 1e3) / HBM_PEAK,
           "of_bare_fill": st["bare_fill"]["median"] / fused, "assembled_over_fused": asm / fused,
           "refresh_assembled_over_fused": st["assembled_add_batch_range_gate_batch_refresh"]["median"] / st["is_less_equal_each_refresh"]["median"],
           "refresh_stats": {name: list(v) for name, v in refreshed.items()},
           "refresh_bytes": nvars * 32, "refresh_bytes_per_s": nvars * 32 / (st["is_less_equal_each_refresh"]["median"] / 1e3),
           "note": "a call's time holds the device check of its arrays (one host synchronisation per call: two in the assembled form) "
                   "and the gather of the assignments; --kernels has the kernels alone"}
    store(args, "emit", out)
    eng.close()


KERNELS_OF_THE_CALLS = ("CompareGateGD", "RangeGateGD", "max_variable_kernel", "gather_wire_values_kernel", "fill_kernel", "gate_batch")


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
    store(args, "kernels", {"tool": "compare_gate_rate --kernels", "source": "rocprofv3 --kernel-trace around --emit", "kernels": rows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emit", action="store_true")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--items-log2", type=int, default=20)
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "compare_gate_rate.json"))
    args = ap.parse_args()
    if args.emit:
        emit(args)
    if args.kernels:
        kernels(args)


if __name__ == "__main__":
    main()
