"""GPU: interval_gate / interval_gate_batch / interval_gate_ragged_batch on the device composer against the Python-integer model
(tests/interval_gate_model.py): every limb of the selector columns, wires and new Variables, materialize's q_range column, check()
and the copy constraints, for every pad (2, 1, 0) with one and with several widget rows, batches that stay inside and cross an
emitter workgroup (256 items), one public pair for the call and a pair per item; the refused calls; clear_witness; the single call;
and one call under a stream that is behind."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth
from tests import interval_gate_model as im

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lagging_stream import LATE, lagging, release  # noqa: E402

R = im.R
S = pg.BlsScalar.from_int
ONE = np.array(synth.mont(1), dtype=np.uint64)
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c")


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def dev_scalars(vals):
    return torch.from_numpy(synth.scalars_from_ints([v % R for v in vals]).view(np.int64)).cuda()


def tv(xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.int64, device="cuda")


def u64(a):
    return np.ascontiguousarray(np.asarray(a)).view(np.uint64)


def witnesses(dev, values):
    """Variables holding `values`, from three kinds of earlier calls: the first of a single add_input, then the even ones of an
    add_input_batch and the odd ones the results of a mul_batch (inputs times a Variable that holds 1)"""
    out = [dev.add_input(S(values[0] % R))]
    rest = list(values[1:])
    ev, od = rest[0::2], rest[1::2]
    tail = [0] * len(rest)
    if ev:
        first = dev.add_input_batch(dev_scalars(ev))
        tail[0::2] = range(first, first + len(ev))
    if od:
        one = dev.add_input(S(1))
        src = dev.add_input_batch(dev_scalars(od))
        res = dev.mul_batch(S(1), tv(range(src, src + len(od))), tv([one] * len(od)), S(0))
        tail[1::2] = res.cpu().tolist()
    return out + tail


def model_of(dev):
    """the model circuit behind the composer as it stands (rows of other calls are not modelled)"""
    vals = [synth.to_int(l) for l in u64(dev.export()["var_values"])]
    return im.Circuit(n_rows=dev.circuit_size(), values=vals, zero_var=dev.zero_var)


def bounds_for(num_bits, n, per_item, rnd):
    """n (lo, hi) pairs: one pair n times, or the edge pairs (lo = 0, lo = hi, the widest interval, hi = r - 1) and random ones"""
    if not per_item:
        lo = rnd.randrange(1, R - 2**num_bits)
        return [(lo, lo + rnd.randrange(2**num_bits))] * n
    out = im.edge_cases(num_bits)
    rnd.shuffle(out)
    while len(out) < n:
        lo = rnd.randrange(R - 2**num_bits)
        out.append((lo, lo + rnd.randrange(2**num_bits)))
    return out[:n]


def inside(bounds, rnd):
    """a witness inside every pair, both ends among them"""
    return [(lo, hi, rnd.randrange(lo, hi + 1))[i % 3] for i, (lo, hi) in enumerate(bounds)]


def mixed(bounds, rnd):
    """roughly every other witness outside its pair: lo - 1, hi + 1, anything"""
    out = inside(bounds, rnd)
    for i, (lo, hi) in enumerate(bounds):
        if i % 2 == 0:
            v = ((lo - 1) % R, (hi + 1) % R, rnd.randrange(R))[(i // 2) % 3]
            out[i] = v
    return out


def append(dev, mod, wv, bounds, num_bits, per_item):
    if per_item:
        dev.interval_gate_ragged_batch(tv(wv), dev_scalars([b[0] for b in bounds]), dev_scalars([b[1] for b in bounds]), num_bits)
    else:
        dev.interval_gate_batch(tv(wv), S(bounds[0][0]), S(bounds[0][1]), num_bits)
    for w, (lo, hi) in zip(wv, bounds):
        mod.interval_gate(w, lo, hi, num_bits)


def compare(dev, mod, n0, nv0):
    got = dev.export(n0, nv0)
    rows, sel = mod.rows[n0:], mod.sel[n0:]
    assert dev.circuit_size() == len(mod.rows) and dev.num_variables() == len(mod.values)
    for j, k in enumerate(SELECTORS):
        assert np.array_equal(u64(got[k]).reshape(-1, 4), synth.scalars_from_ints([s[j] for s in sel])), k
    for j, k in enumerate(("w_l", "w_r", "w_o")):
        assert np.array_equal(u64(got[k]), np.array([r[j] for r in rows], dtype=np.uint64)), k
    assert np.array_equal(u64(got["var_values"]).reshape(-1, 4), synth.scalars_from_ints(mod.values[nv0:])), "var_values"


def q_range_expected(mod):
    exp = np.zeros((len(mod.rows), 4), dtype=np.uint64)
    exp[np.array(mod.q_range, dtype=bool)] = ONE
    return exp


@pytest.mark.parametrize("per_item", (False, True), ids=("uniform", "per_item"))
@pytest.mark.parametrize("batch", (1, 3, 257))
@pytest.mark.parametrize("num_bits", im.NUM_BITS)
def test_emission_materialize_and_check(engine, num_bits, batch, per_item):
    rnd = random.Random(num_bits * 1000 + batch * 2 + per_item)
    k, g, pad = im.layout(num_bits)
    dev = pg.StandardComposer(engine, gate_capacity=1 << 16, var_capacity=1 << 18)
    b_good, b_mixed = bounds_for(num_bits, batch, per_item, rnd), bounds_for(num_bits, batch, per_item, rnd)
    good, bad = inside(b_good, rnd), mixed(b_mixed, rnd)
    wv = witnesses(dev, good + bad)
    mod = model_of(dev)
    n0, nv0 = dev.circuit_size(), dev.num_variables()

    # every witness inside its interval
    append(dev, mod, wv[:batch], b_good, num_bits, per_item)
    compare(dev, mod, n0, nv0)
    assert dev.circuit_size() == n0 + batch * 2 * (g + 1) and dev.num_variables() == nv0 + batch * 2 * k
    assert mod.first_bad() == -1 and dev.check() == -1
    assert dev.copy_constraints_hold()
    full = dev.materialize()
    assert np.array_equal(u64(full["q_range"].cpu().numpy()), q_range_expected(mod))
    assert (u64(full["q_arith"].cpu().numpy()) == ONE).all()
    del full

    # a second call right behind the first (one range segment), every other witness outside: all their rows, and check names the
    # model's first failing row (row 0 of the half whose difference is negative)
    n1, nv1 = dev.circuit_size(), dev.num_variables()
    append(dev, mod, wv[batch:], b_mixed, num_bits, per_item)
    compare(dev, mod, n1, nv1)
    bad_row = mod.first_bad()
    assert bad_row >= n1 and (bad_row - n1) % (g + 1) == 0
    assert dev.check() == bad_row
    assert dev.copy_constraints_hold()
    assert np.array_equal(u64(dev.materialize()["q_range"].cpu().numpy()), q_range_expected(mod))
    dev.close()


def test_the_single_call_equals_a_batch_of_one(engine):
    cases = [(8, 100, 300, 255), (62, 0, 2**62 - 1, 0), (2, R - 4, R - 1, R - 1), (252, 5, 5 + 2**252 - 1, 2**251), (64, 7, 7, 7)]
    a, b = pg.StandardComposer(engine), pg.StandardComposer(engine)
    wa = [a.add_input(S(v)) for _, _, _, v in cases]
    wb = [b.add_input(S(v)) for _, _, _, v in cases]
    mod = model_of(a)
    n0, nv0 = a.circuit_size(), a.num_variables()
    for (bits, lo, hi, _), x, y in zip(cases, wa, wb):
        a.interval_gate(x, S(lo), S(hi), bits)
        b.interval_gate_batch(tv([y]), S(lo), S(hi), bits)
        mod.interval_gate(x, lo, hi, bits)
    compare(a, mod, n0, nv0)
    ea, eb = a.export(), b.export()
    for k in ea:
        assert np.array_equal(u64(ea[k]), u64(eb[k])), k
    assert a.check() == -1 and a.copy_constraints_hold()
    assert torch.equal(a.materialize()["q_range"], b.materialize()["q_range"])
    assert np.array_equal(u64(a.materialize()["q_range"].cpu().numpy()), q_range_expected(mod))
    # out by one on either side
    for v, half in ((99, 0), (301, 1)):
        row = a.circuit_size()
        a.interval_gate(a.add_input(S(v)), S(100), S(300), 8)
        assert a.check() == row + half * 3
        a.close()
        a = pg.StandardComposer(engine)
    a.close()
    b.close()


def test_refused_calls_append_nothing(engine):
    dev = pg.StandardComposer(engine)
    first = dev.add_input_batch(dev_scalars([1, 2, 3, 4, 5]))
    state = (dev.circuit_size(), dev.num_variables())
    good = tv(range(first, first + 5))
    lo5, hi5 = dev_scalars([0, 1, 2, 3, 4]), dev_scalars([10, 11, 12, 13, 14])

    def refused(match, call, *args):
        with pytest.raises(pg.PgError, match=match) as e:
            call(*args)
        assert e.value.status == 2
        assert (dev.circuit_size(), dev.num_variables()) == state

    for bits in (0, 1, 7, 253, 254, 256, 2**32 + 8):
        refused("num_bits", dev.interval_gate_batch, good, S(0), S(3), bits)
        refused("num_bits", dev.interval_gate, first, S(0), S(3), bits)
        refused("num_bits", dev.interval_gate_ragged_batch, good, lo5, hi5, bits)
    for lo, hi, bits in ((6, 5, 8), (R - 1, 0, 8), (0, 256, 8), (1, R - 1, 252), (0, 4, 2)):
        refused("interval_gate", dev.interval_gate_batch, good, S(lo), S(hi), bits)
        refused("interval_gate", dev.interval_gate, first, S(lo), S(hi), bits)
    # per item: the message names the FIRST item whose pair violates a precondition
    for bad_items, bits in ((((3, 6, 5),), 8), (((1, 0, 256), (4, 9, 8)), 8), (((4, R - 1, 0), (2, 0, 2**64)), 64), (((0, 0, 4),), 2)):
        lo, hi = [0, 1, 2, 3, 4], [3, 3, 3, 3, 4]
        for i, l, h in bad_items:
            lo[i], hi[i] = l, h
        refused(f"first is item {min(b[0] for b in bad_items)}\\b", dev.interval_gate_ragged_batch, good, dev_scalars(lo), dev_scalars(hi), bits)
    # a bound that is not reduced below the modulus (raw limbs of r itself)
    raw = hi5.clone()
    raw[2] = torch.from_numpy(np.array([R >> (64 * j) & (2**64 - 1) for j in range(4)], dtype=np.uint64).view(np.int64)).cuda()
    refused("first is item 2", dev.interval_gate_ragged_batch, good, lo5, raw, 64)
    nv = dev.num_variables()
    refused("unknown Variable", dev.interval_gate_batch, tv([first, nv, first + 1]), S(0), S(3), 8)
    refused("unknown Variable", dev.interval_gate_ragged_batch, tv([first, nv, first + 1, first, first]), lo5, hi5, 8)
    refused("unknown Variable", dev.interval_gate, nv, S(0), S(3), 8)
    with pytest.raises(ValueError):
        dev.interval_gate_ragged_batch(good, lo5[:4], hi5, 8)
    lib = dev._lib
    assert lib.pg_composer_interval_gate_batch(None, good.data_ptr(), S(0).c, S(3).c, 8, 5) == 2
    assert lib.pg_composer_interval_gate_batch(dev._h, None, S(0).c, S(3).c, 8, 5) == 2
    assert lib.pg_composer_interval_gate_batch(dev._h, good.data_ptr(), None, S(3).c, 8, 5) == 2
    assert lib.pg_composer_interval_gate_ragged_batch(dev._h, good.data_ptr(), None, hi5.data_ptr(), 8, 5) == 2
    assert lib.pg_composer_interval_gate_ragged_batch(None, good.data_ptr(), lo5.data_ptr(), hi5.data_ptr(), 8, 5) == 2
    assert lib.pg_composer_interval_gate(None, 0, S(0).c, S(3).c, 8) == 2
    assert (dev.circuit_size(), dev.num_variables()) == state and dev.check() == -1
    assert not dev.materialize()["q_range"].any()
    dev.interval_gate_batch(good[:0], S(0), S(3), 8)  # an empty batch is nothing
    dev.interval_gate_ragged_batch(good[:0], lo5[:0], hi5[:0], 8)
    assert (dev.circuit_size(), dev.num_variables()) == state
    # and the composer still works: the widest legal pairs are taken
    dev.interval_gate_ragged_batch(good, lo5, dev_scalars([255, 256, 257, 258, 259]), 8)
    assert dev.check() == -1
    dev.close()


def test_clear_witness_finds_the_rows_in_place(engine):
    """after clear_witness the same calls with other witnesses write assignments only (refresh_stats) and the composer equals a
    fresh build of the second witnesses; the same calls with ONE bound moved are not taken for the same calls"""
    rnd = random.Random(5)
    n_a, n_b = 300, 40
    lo_b = [rnd.randrange(2**40) for _ in range(n_b)]
    hi_b = [lo + rnd.randrange(2**16) for lo in lo_b]

    def program(dev, values, uniform=(1000, 1000 + 2**62 - 2), hi=hi_b):
        wv = witnesses(dev, values)
        dev.interval_gate_batch(tv(wv[:n_a]), S(uniform[0]), S(uniform[1]), 62)
        dev.interval_gate_ragged_batch(tv(wv[n_a:]), dev_scalars(lo_b), dev_scalars(hi), 16)
        dev.interval_gate(wv[0], S(0), S(2**64 - 1), 64)
        dev.interval_gate(wv[n_a], S(lo_b[0]), S(lo_b[0] + 3), 2)
        return wv

    def values():
        return [rnd.randrange(1000, 1000 + 2**62 - 2) for _ in range(n_a)] + [lo_b[0] + rnd.randrange(min(4, hi_b[0] - lo_b[0] + 1))] + \
            [rnd.randrange(lo, hi + 1) for lo, hi in zip(lo_b[1:], hi_b[1:])]

    dev = pg.StandardComposer(engine, 1 << 15, 1 << 16)
    program(dev, values())
    n_rows = dev.circuit_size()
    assert dev.check() == -1
    dev.clear_witness()
    second = values()
    program(dev, second)
    kept, rewritten, refreshing = dev.refresh_stats()
    assert (kept, rewritten, refreshing) == (n_rows - 3, 0, True)
    kept_all = kept
    fresh = pg.StandardComposer(engine, 1 << 15, 1 << 16)
    wv = program(fresh, second)
    a, b = dev.export(), fresh.export()
    for k in a:
        assert np.array_equal(u64(a[k]), u64(b[k])), k
    assert dev.check() == -1 and dev.copy_constraints_hold()
    assert torch.equal(dev.materialize()["q_range"], fresh.materialize()["q_range"])
    # the refreshed values are the model's
    vals = [synth.to_int(l) for l in u64(a["var_values"])]
    nv0 = dev.num_variables() - (n_a * 62 + n_b * 16 + 64 + 2)
    mod = im.Circuit(n_rows=0, values=vals[:nv0], zero_var=dev.zero_var)
    for w in wv[:n_a]:
        mod.interval_gate(w, 1000, 1000 + 2**62 - 2, 62)
    for w, lo, hi in zip(wv[n_a:], lo_b, hi_b):
        mod.interval_gate(w, lo, hi, 16)
    mod.interval_gate(wv[0], 0, 2**64 - 1, 64)
    mod.interval_gate(wv[n_a], lo_b[0], lo_b[0] + 3, 2)
    assert mod.values == vals and mod.first_bad() == -1
    # other witnesses, one of them outside: its rows are still in place, and check names row 0 of its upper half
    dev.clear_witness()
    third = values()
    third[7] = 1000 + 2**62 - 1  # (max + 1; max - min is one short of the widest, so the lower half still holds)
    program(dev, third)
    assert dev.refresh_stats() == (kept_all, 0, True)
    first_interval_row = n_rows - (n_a * 2 * 12 + n_b * 2 * 4 + 2 * 12 + 2 * 2)
    assert dev.check() == first_interval_row + 7 * 24 + 12
    # one uniform bound moved by one: from that call on the rows are written again
    dev.clear_witness()
    program(dev, second, uniform=(1000, 1000 + 2**62 - 3))
    kept, rewritten, refreshing = dev.refresh_stats()
    assert not refreshing and rewritten == n_rows - first_interval_row and kept == kept_all - rewritten
    moved = pg.StandardComposer(engine, 1 << 15, 1 << 16)
    program(moved, second, uniform=(1000, 1000 + 2**62 - 3))
    a, b = dev.export(), moved.export()
    for k in a:
        assert np.array_equal(u64(a[k]), u64(b[k])), k
    moved.close()
    # one per-item bound moved by one: the uniform call before it is found in place, the per-item call is not
    dev.clear_witness()
    hi_moved = list(hi_b)
    hi_moved[n_b // 2] += 1
    program(dev, second, uniform=(1000, 1000 + 2**62 - 3), hi=hi_moved)
    kept, rewritten, refreshing = dev.refresh_stats()
    assert not refreshing and rewritten == n_b * 2 * 4 + 2 * 12 + 2 * 2
    moved = pg.StandardComposer(engine, 1 << 15, 1 << 16)
    program(moved, second, uniform=(1000, 1000 + 2**62 - 3), hi=hi_moved)
    a, b = dev.export(), moved.export()
    for k in a:
        assert np.array_equal(u64(a[k]), u64(b[k])), k
    assert dev.check() == -1
    moved.close()
    dev.close()
    fresh.close()


@pytest.mark.parametrize("per_item", (False, True), ids=("uniform", "per_item"))
def test_interval_gate_batch_under_a_lagging_stream(engine, per_item):
    """a composer made on the default stream; the array of Variables (and the per-item bounds) are filled in on a side stream that
    is behind: while the host issues the call they hold other Variables and other (valid) bounds"""
    num_bits, batch = 16, 40
    rng = random.Random(78)
    side = torch.cuda.Stream()
    lo = [rng.randrange(2**30) for _ in range(batch)] if per_item else [12345] * batch
    hi = [l + rng.randrange(2**num_bits) for l in lo] if per_item else [12345 + 2**num_bits - 1] * batch
    values = [rng.randrange(l, h + 1) for l, h in zip(lo, hi)]
    stale_values = [l + 70000 for l in lo]  # inside the stale bounds alone
    comp = pg.StandardComposer(engine, 1 << 12, 1 << 13)
    first = comp.add_input_batch(dev_scalars(values + stale_values))
    mod = model_of(comp)
    n0, nv0 = comp.circuit_size(), comp.num_variables()
    true, stale = list(range(first, first + batch)), list(range(first + batch, first + 2 * batch))
    t_true, t_lo, t_hi = tv(true), dev_scalars(lo), dev_scalars(hi)
    s_lo, s_hi = dev_scalars([l + 65536 for l in lo]), dev_scalars([h + 65536 for h in hi])
    wv, b_lo, b_hi = tv(stale), s_lo.clone(), s_hi.clone()

    def call(c):
        if per_item:
            c.interval_gate_ragged_batch(wv, b_lo, b_hi, num_bits)
        else:
            c.interval_gate_batch(wv, S(lo[0]), S(hi[0]), num_bits)
    c0 = pg.StandardComposer(engine, 1 << 12, 1 << 13)  # warm-up on another composer, under both streams
    c0.add_input_batch(dev_scalars(values + stale_values))
    call(c0)
    with torch.cuda.stream(side):
        call(c0)
    c0.sync()
    c0.close()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            ev = lagging(side)
            wv.copy_(t_true)
            b_lo.copy_(t_lo)
            b_hi.copy_(t_hi)
            assert not ev.query(), LATE
            call(comp)  # (it checks its arrays first: a host synchronisation)
            got_check = comp.check()
        torch.cuda.synchronize()
        for w, l, h in zip(true, lo, hi):
            mod.interval_gate(w, l, h, num_bits)
        compare(comp, mod, n0, nv0)
        assert got_check == -1 and mod.first_bad() == -1
        assert np.array_equal(u64(comp.materialize()["q_range"].cpu().numpy()), q_range_expected(mod))
    finally:
        release()
        comp.close()
