#!/usr/bin/env python3
"""uniform vs ragged range_check on the same witnesses with ONE (0, 2^254) pair for every item: what do the per-item
entry points cost when nothing is ragged?  (1 GPU; the counterpart of tools/time_max_bound.py for the two-block item.)

Both forms write the same bytes into the same output buffer; the ragged plan is made once, outside the timed window, as a
caller that reuses the plan of its public bounds would.  The two are timed alternately in one process: a warm-up call each, then
REPS calls each, device events around every call.  Prints one JSON line (and writes it to the file given as argument)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth

REPS = 9
dev = torch.device("cuda", 0)
eng = pg.Engine(0)
mn, mx = pg.BlsScalar.from_int(0), pg.BlsScalar.from_int(1 << 254)
per_item = eng.range_check_layout(mn, mx, 1)
item_bytes = per_item.n_gates * 184 + per_item.n_vars * 32
# the largest power of two of items whose output (one buffer, written by both forms) and inputs fit the free memory
free = torch.cuda.mem_get_info(dev)[0]
batch = 1 << 20
while batch > 1024 and batch * (item_bytes + 4 * 32 + 24) > 0.9 * free:
    batch >>= 1
lay = eng.range_check_layout(mn, mx, batch)
nbytes = lay.n_gates * 184 + lay.n_vars * 32
wit = torch.from_numpy(np.ascontiguousarray(synth.random_scalars(batch)).view(np.int64)).to(dev)
mins = torch.from_numpy(np.repeat(synth.scalars_from_ints([0]), batch, axis=0).view(np.int64)).to(dev)
maxs = torch.from_numpy(np.repeat(synth.scalars_from_ints([1 << 254]), batch, axis=0).view(np.int64)).to(dev)
cols = pg.Columns.allocate(lay.n_gates, lay.n_vars, dev)
res = torch.empty((batch,), dtype=torch.int64, device=dev)
nb, roff, voff = eng.ragged_buffers(batch)
plan = eng.range_check_ragged_plan(maxs, nb, roff, voff)
assert (plan.n_gates, plan.n_vars) == (lay.n_gates, lay.n_vars)
stream = torch.cuda.current_stream(dev)


def uniform():
    eng.range_check_batch(mn, mx, wit, 3, 5, out=cols, result_vars=res)


def ragged():
    eng.range_check_ragged_emit(mins, maxs, wit, nb, roff, voff, cols, res, 3, 5)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


# the two forms write the same table: compare before timing (a sample of rows and the whole variable table's checksum)
uniform()
torch.cuda.synchronize()
probe = (cols.q_c[:4096].clone(), cols.w_o[-4096:].clone(), int(cols.var_values.sum()))
cols.var_values.zero_()
ragged()
torch.cuda.synchronize()
assert torch.equal(probe[0], cols.q_c[:4096]) and torch.equal(probe[1], cols.w_o[-4096:]) and probe[2] == int(cols.var_values.sum())
times = {"uniform": [], "ragged": []}
for _ in range(REPS):
    times["uniform"].append(once(uniform))
    times["ragged"].append(once(ragged))
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
out = {
    "what": "pg_range_check_batch vs pg_range_check_ragged_batch, (min, max) = (0, 2^254) for every item, same witnesses, same output buffer",
    "device": torch.cuda.get_device_name(dev), "batch": batch, "num_bits": lay.num_bits, "bytes": nbytes, "reps": REPS,
    "uniform_ms": round(med["uniform"], 3), "ragged_ms": round(med["ragged"], 3),
    "uniform_ms_min_max": [round(min(times["uniform"]), 3), round(max(times["uniform"]), 3)],
    "ragged_ms_min_max": [round(min(times["ragged"]), 3), round(max(times["ragged"]), 3)],
    "uniform_GBps": round(nbytes / med["uniform"] / 1e6, 1), "ragged_GBps": round(nbytes / med["ragged"] / 1e6, 1),
    "ragged_over_uniform_time": round(med["ragged"] / med["uniform"], 4),
}
line = json.dumps(out)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
