"""The figures of DESIGN section 3.22 (they need the GPU): weighted_sum_ragged_batch on three workloads, one process, every repetition
on a fresh composer with a host clock around the call and a synchronise (the call checks its arrays, gathers the assignments, and
runs its three launches), medians and ranges after a warm-up -> one JSON line, stored in --out (default
profiles/weighted_sum_rate.json):

  a   2^20 segments of uniformly 2 .. 16 terms, and its values-only refresh after clear_witness
  b   one segment of 2^24 terms
  c   2^22 segments of 2 terms, and ONE add_batch of 2^22 items (the same rows with one set of selectors)
  m4  2^20 segments of 4 terms, and the three chained add_batch calls that state the same thing (uniform selectors)

each with coefficients and constants and without either, and beside each the bare fill of the bytes it writes (184 a row, 32 a
Variable).  --only a,b,... picks workloads (a run under rocprofv3 --kernel-trace --stats takes `--only a`); --scale-log2 k shrinks
every workload by 2^k (a dry run).
usage: python tools/weighted_sum_rate.py [--reps 5] [--warmup 1] [--only a,b,c,m4] [--scale-log2 0] [--out F]"""
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
DEV = "cuda:0"
POOL = 1 << 16        # input Variables the terms are drawn from


def stats(v):
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def timed_once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def repeated(base, n):
    return base.repeat((n + base.shape[0] - 1) // base.shape[0], 1)[:n].contiguous()


def scalars(n, seed):
    """n reduced pseudo-random scalars on the device (4096 distinct ones, repeated: the stores do not depend on them)"""
    return repeated(torch.from_numpy(synth.random_scalars(min(n, 4096), seed).view(np.int64)).to(DEV), n)


def workload(name, shrink):
    rnd = np.random.default_rng(11)
    if name == "a":
        sizes = rnd.integers(2, 17, (1 << 20) >> shrink)
    elif name == "b":
        sizes = np.array([(1 << 24) >> shrink])
    elif name == "c":
        sizes = np.full((1 << 22) >> shrink, 2)
    else:
        sizes = np.full((1 << 20) >> shrink, 4)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return torch.from_numpy(off).to(DEV), int(off[-1]), len(sizes)


def measure(eng, name, args):
    seg_off, terms, segments = workload(name, args.scale_log2)
    rows = terms - segments
    nbytes = rows * (184 + 32)
    pool_vals = scalars(POOL, 5)
    idx = torch.randint(0, POOL, (terms,), device=DEV, dtype=torch.int64)
    co, ks = scalars(terms, 6), scalars(segments, 7)
    buf = torch.empty(((nbytes + 15) // 16 * 16,), dtype=torch.uint8, device=DEV)   # (the fill moves 16 bytes a lane)

    def fresh():
        comp = pg.StandardComposer(eng, rows + 16, rows + POOL + 16)
        first = comp.add_input_batch(pool_vals)
        comp.sync()
        return comp, first

    forms = {"with_coeffs": lambda comp, x: comp.weighted_sum_ragged_batch(x, seg_off, co, ks),
             "without_coeffs": lambda comp, x: comp.weighted_sum_ragged_batch(x, seg_off)}
    if name == "c":       # the same rows from one add_batch: pairs (x[2s], x[2s + 1])
        forms["add_batch"] = lambda comp, x: comp.add_batch(S(3), x[0::2].contiguous(), S(5), x[1::2].contiguous(), S(7))
    if name == "m4":      # ((x0 + x1) + x2) + x3 by three add_batch calls
        def chain(comp, x):
            acc = comp.add_batch(S(3), x[0::4].contiguous(), S(5), x[1::4].contiguous(), S(7))
            acc = comp.add_batch(S(1), acc, S(5), x[2::4].contiguous(), S(0))
            comp.add_batch(S(1), acc, S(5), x[3::4].contiguous(), S(0))
        forms["add_batch_x3"] = chain
    ms = {k: [] for k in forms}
    ms["bare_fill"] = []
    if name == "a":
        ms.update({"with_coeffs_refresh": [], "without_coeffs_refresh": []})
    for rep in range(args.warmup + args.reps):
        for form in (list(forms) if rep % 2 == 0 else list(forms)[::-1]):
            comp, first = fresh()
            x = first + idx
            t_full = timed_once(lambda: forms[form](comp, x))
            assert comp.circuit_size() - 3 == rows, (name, form, comp.circuit_size())
            t_ref = None
            if name == "a" and form in ("with_coeffs", "without_coeffs"):
                comp.clear_witness()
                comp.add_input_batch(pool_vals)
                comp.sync()
                t_ref = timed_once(lambda: forms[form](comp, x))
                assert comp.refresh_stats() == (rows, 0, True), comp.refresh_stats()
            if rep == args.warmup + args.reps - 1:
                assert comp.check() == -1, (name, form)
            comp.close()
            del comp, x
            torch.cuda.empty_cache()
            t_fill = timed_once(lambda: eng.fill_bytes(buf))
            if rep >= args.warmup:
                ms[form].append(t_full)
                ms["bare_fill"].append(t_fill)
                if t_ref is not None:
                    ms[form + "_refresh"].append(t_ref)
    st = {k: stats(v) for k, v in ms.items()}
    out = {"terms": terms, "segments": segments, "rows": rows, "bytes_written": nbytes, "ms": st,
           "bytes_per_s": {k: nbytes / (st[k]["median"] / 1e3) for k in forms},
           "of_bare_fill": {k: st["bare_fill"]["median"] / st[k]["median"] for k in forms},
           "ns_per_row": {k: st[k]["median"] * 1e6 / rows for k in forms}}
    if name == "a":
        out["refresh_bytes"] = rows * 32
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="a,b,c,m4")
    ap.add_argument("--scale-log2", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "weighted_sum_rate.json"))
    args = ap.parse_args()
    eng = pg.Engine(0)
    out = {"tool": "weighted_sum_rate", "reps": args.reps, "warmup": args.warmup, "scale_log2": args.scale_log2, "workloads": {}}
    for name in args.only.split(","):
        out["workloads"][name] = measure(eng, name, args)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()
