"""GPU: is_less_equal / is_less_equal_each on the device composer against the Python-integer model (tests/compare_gate_model.py):
every limb of the five selector columns, the three wire columns and the new Variables, result_vars, materialize's q_range column
with a sentinel row behind it, check() against the model's first failing row and the copy constraints, for every pad with one and
with several widget rows, batches that stay inside and cross an emitter workgroup (256 items), both `strict` values; inputs that are
results of range_gate_batch, add_batch and add_input_batch, zero_var on either side, one Variable on both; the refused calls; the
single call; and one call under a stream that is behind."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import _lib, synth
from tests import compare_gate_model as cm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lagging_stream import LATE, lagging, release  # noqa: E402

R = cm.R
S = pg.BlsScalar.from_int
ONE = np.array(synth.mont(1), dtype=np.uint64)
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c")
SENTINEL = -7


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


def model_of(dev):
    """the model circuit behind the composer as it stands (rows of other calls are not modelled)"""
    vals = [synth.to_int(l) for l in u64(dev.export()["var_values"])]
    return cm.Circuit(n_rows=dev.circuit_size(), values=vals, zero_var=dev.zero_var)


def pairs_of_values(num_bits, n, rnd):
    """n (x, y) below 2^num_bits: x > y, x = y, x < y in turn, the extremes among them"""
    top = 2**num_bits - 1
    out = []
    for i in range(n):
        a, b = sorted((rnd.randrange(top + 1), rnd.randrange(top + 1)))
        if a == b:
            a, b = 0, top
        if i < 3:
            a, b = 0, top
        elif i < 6:
            a = b - 1
        out.append(((b, a), (b, b), (a, b))[i % 3])
    return out


def inputs(dev, num_bits, values):
    """-> (pairs of Variables holding `values`, specials).  x of the even items and every y come from an add_input_batch; x of the
    odd items is the result of an add_batch (1 * x + 0 * x).  specials: two accumulators of a range_gate_batch (values below 4), and a
    Variable that holds 3 * 2^num_bits + 1"""
    n = len(values)
    first = dev.add_input_batch(dev_scalars([x for x, _ in values] + [y for _, y in values] + [13, 6, 3 * 2**num_bits + 1]))
    xs, ys = list(range(first, first + n)), list(range(first + n, first + 2 * n))
    copies = dev.add_batch(S(1), tv(xs), S(0), tv(xs), S(0)).cpu().tolist()
    xs[1::2] = copies[1::2]
    acc0 = dev.num_variables()
    dev.range_gate_batch(tv([first + 2 * n, first + 2 * n + 1]), 4)     # one accumulator each: 13 >> 2 = 3, 6 >> 2 = 1
    assert dev.num_variables() == acc0 + 2
    return list(zip(xs, ys)), {"acc_hi": acc0, "acc_lo": acc0 + 1, "big": first + 2 * n + 2}


def append(dev, mod, pairs, num_bits, strict):
    """one is_less_equal_each on the device and, item by item, on the model; result_vars compared"""
    res = dev.is_less_equal_each(tv([x for x, _ in pairs]), tv([y for _, y in pairs]), num_bits, strict)
    exp = [mod.is_less_equal(x, y, num_bits, strict)[1] for x, y in pairs]
    assert res.cpu().tolist() == exp
    return exp


def compare(dev, mod, n0, nv0):
    got = dev.export(n0, nv0)
    rows, sel = mod.rows[n0:], mod.sel[n0:]
    assert dev.circuit_size() == len(mod.rows) and dev.num_variables() == len(mod.values)
    for j, k in enumerate(SELECTORS):
        assert np.array_equal(u64(got[k]).reshape(-1, 4), synth.scalars_from_ints([s[j] for s in sel])), k
    for j, k in enumerate(("w_l", "w_r", "w_o")):
        assert np.array_equal(u64(got[k]), np.array([r[j] for r in rows], dtype=np.uint64)), k
    assert np.array_equal(u64(got["var_values"]).reshape(-1, 4), synth.scalars_from_ints(mod.values[nv0:])), "var_values"


def q_range_of(dev):
    return u64(dev.materialize()["q_range"].cpu().numpy())


def assert_q_range(dev, mod, head=None):
    """q_range materialised alone into a buffer with a sentinel row behind it, and with every other column.  head: the column as it
    was before the rows the model has (range_gate rows among the rows of other calls, which the model does not know)"""
    n = dev.circuit_size()
    exp = np.zeros((n, 4), dtype=np.uint64)
    exp[np.array(mod.q_range, dtype=bool)] = ONE
    if head is not None:
        exp[:len(head)] = head
    alone = torch.full((n + 1, 4), -1, dtype=torch.int64, device="cuda")
    assert dev._lib.pg_composer_materialize(dev._h, C.byref(_lib.FullColumnsC(q_range=alone.data_ptr()))) == 0
    assert np.array_equal(u64(alone[:-1].cpu().numpy()), exp)
    assert (alone[-1] == -1).all()
    assert np.array_equal(u64(dev.materialize()["q_range"].cpu().numpy()), exp)


@pytest.mark.parametrize("strict", (False, True), ids=("le", "lt"))
@pytest.mark.parametrize("batch", (1, 3, 257))
@pytest.mark.parametrize("num_bits", cm.NUM_BITS)
def test_emission_materialize_and_check(engine, num_bits, batch, strict):
    rnd = random.Random(num_bits * 1000 + batch * 2 + strict)
    k, g, pad = cm.layout(num_bits)
    dev = pg.StandardComposer(engine, gate_capacity=1 << 15, var_capacity=1 << 17)
    values = pairs_of_values(num_bits, 2 * batch, rnd)
    pairs, sp = inputs(dev, num_bits, values)
    first, second = pairs[:batch], pairs[batch:]
    zero = dev.zero_var
    if batch >= 3:
        first[0] = (zero, first[0][1])               # zero_var as x
        first[1] = (first[1][0], first[1][0])        # one Variable as x and as y
        first[2] = (sp["acc_hi"], sp["acc_lo"])      # results of range_gate_batch: 3 against 1
        second[0] = (second[0][0], zero)             # zero_var as y
        second[1] = (sp["acc_lo"], sp["acc_hi"])
        second[batch // 2 + 1] = (zero, sp["big"])   # planted: z = 2^(num_bits + 2) + 1 - strict does not fit the widget
    mod = model_of(dev)
    n0, nv0 = dev.circuit_size(), dev.num_variables()
    head = q_range_of(dev)
    assert head.shape == (n0, 4) and head.any()      # (the two range_gate items that made the accumulators)

    # every item holds
    res = append(dev, mod, first, num_bits, strict)
    compare(dev, mod, n0, nv0)
    assert dev.circuit_size() == n0 + batch * (g + 1) and dev.num_variables() == nv0 + batch * k
    assert res == [nv0 + i * k for i in range(batch)]
    for (xv, yv), r in zip(first, res):
        x, y = mod.values[xv], mod.values[yv]
        assert mod.values[r] == int(x < y if strict else x <= y), (x, y)
    if batch >= 3:
        assert sum(mod.values[x] > mod.values[y] for x, y in first) >= batch // 3 - 1
        assert sum(mod.values[x] == mod.values[y] for x, y in first) >= batch // 3 - 1
    assert mod.first_bad() == -1 and dev.check() == -1
    assert dev.copy_constraints_hold()
    assert_q_range(dev, mod, head)

    # a second call right behind the first (one range segment), one item planted out of range in the larger batches: all its rows, and
    # check names the model's first failing row, the item's row 0
    n1, nv1 = dev.circuit_size(), dev.num_variables()
    append(dev, mod, second, num_bits, strict)
    compare(dev, mod, n1, nv1)
    bad_row = mod.first_bad()
    assert bad_row == (n1 + (batch // 2 + 1) * (g + 1) if batch >= 3 else -1)
    assert dev.check() == bad_row
    assert dev.copy_constraints_hold()
    assert_q_range(dev, mod, head)
    dev.close()


def test_the_single_call_equals_a_batch_of_one(engine):
    cases = [(8, 100, 255, False), (62, 0, 2**62 - 1, True), (2, 3, 3, False), (2, 3, 3, True), (252, 2**252 - 1, 2**251, False),
             (64, 7, 7, True), (4, 9, 8, False)]
    a, b = pg.StandardComposer(engine), pg.StandardComposer(engine)
    va = [(a.add_input(S(x)), a.add_input(S(y))) for _, x, y, _ in cases]
    vb = [(b.add_input(S(x)), b.add_input(S(y))) for _, x, y, _ in cases]
    mod = model_of(a)
    n0, nv0 = a.circuit_size(), a.num_variables()
    for (bits, x, y, strict), (xa, ya), (xb, yb) in zip(cases, va, vb):
        got = a.is_less_equal(xa, ya, bits, strict)
        rb = b.is_less_equal_each(tv([xb]), tv([yb]), bits, strict)
        _, exp = mod.is_less_equal(xa, ya, bits, strict)
        assert got == exp == int(rb[0])
        assert mod.values[exp] == int(x < y if strict else x <= y)
    assert a.is_less_equal(va[0][0], va[0][0], 8) == mod.is_less_equal(va[0][0], va[0][0], 8)[1]      # one Variable on both sides
    b.is_less_equal_each(tv([vb[0][0]]), tv([vb[0][0]]), 8)
    compare(a, mod, n0, nv0)
    ea, eb = a.export(), b.export()
    for k in ea:
        assert np.array_equal(u64(ea[k]), u64(eb[k])), k
    assert a.check() == -1 and a.copy_constraints_hold()
    assert torch.equal(a.materialize()["q_range"], b.materialize()["q_range"])
    assert_q_range(a, mod)
    row = a.circuit_size()
    a.is_less_equal(a.zero_var, a.add_input(S(3 * 2**8)), 8)
    assert a.check() == row
    a.close()
    b.close()


def test_refused_calls_append_nothing_and_leave_the_results_alone(engine):
    dev = pg.StandardComposer(engine)
    first = dev.add_input_batch(dev_scalars([1, 2, 3, 4, 5]))
    state = (dev.circuit_size(), dev.num_variables())
    good, other = tv(range(first, first + 5)), tv([first + 4, first, first, first + 2, first + 1])
    res = torch.full((5,), SENTINEL, dtype=torch.int64, device="cuda")
    lib = dev._lib

    def untouched():
        assert (res == SENTINEL).all()
        assert (dev.circuit_size(), dev.num_variables()) == state

    def refused(match, call, *args):
        with pytest.raises(pg.PgError, match=match) as e:
            call(*args)
        assert e.value.status == 2
        untouched()

    for bits in (0, 1, 7, 63, 253, 254, 256, 2**32 + 8):
        refused("num_bits", dev.is_less_equal_each, good, other, bits)
        refused("num_bits", dev.is_less_equal, first, first + 1, bits, True)
        assert lib.pg_composer_is_less_equal_batch(dev._h, good.data_ptr(), other.data_ptr(), bits, 0, 5, res.data_ptr()) == 2
        untouched()
    nv = dev.num_variables()
    for x, y in ((tv([first, nv, first + 1, first, first]), good), (good, tv([first, first, first, first, nv + 7]))):
        refused("unknown Variable", dev.is_less_equal_each, x, y, 8)
        assert lib.pg_composer_is_less_equal_batch(dev._h, x.data_ptr(), y.data_ptr(), 8, 1, 5, res.data_ptr()) == 2
        untouched()
    refused("unknown Variable", dev.is_less_equal, nv, first, 8)
    refused("unknown Variable", dev.is_less_equal, first, nv, 8)
    with pytest.raises(ValueError):
        dev.is_less_equal_each(good, other[:4], 8)
    out = C.c_uint64(12345)
    assert lib.pg_composer_is_less_equal_batch(None, good.data_ptr(), other.data_ptr(), 8, 0, 5, res.data_ptr()) == 2
    assert lib.pg_composer_is_less_equal_batch(dev._h, None, other.data_ptr(), 8, 0, 5, res.data_ptr()) == 2
    assert lib.pg_composer_is_less_equal_batch(dev._h, good.data_ptr(), None, 8, 0, 5, res.data_ptr()) == 2
    assert lib.pg_composer_is_less_equal(None, first, first + 1, 8, 0, C.byref(out)) == 2
    assert lib.pg_composer_is_less_equal(dev._h, first, first + 1, 8, 0, None) == 2
    assert lib.pg_composer_is_less_equal(dev._h, first, first + 1, 9, 0, C.byref(out)) == 2
    assert lib.pg_composer_is_less_equal(dev._h, first, nv, 8, 0, C.byref(out)) == 2
    assert out.value == 12345
    untouched()
    assert dev.check() == -1 and not dev.materialize()["q_range"].any()
    assert dev.is_less_equal_each(good[:0], other[:0], 8).shape == (0,)     # an empty batch is nothing
    untouched()
    # and the composer still works; result_vars may be NULL
    assert lib.pg_composer_is_less_equal_batch(dev._h, good.data_ptr(), other.data_ptr(), 8, 0, 5, None) == 0
    assert lib.pg_composer_is_less_equal_batch(dev._h, good.data_ptr(), other.data_ptr(), 8, 1, 5, res.data_ptr()) == 0
    k, g, _ = cm.layout(8)
    assert res.cpu().tolist() == [state[1] + (5 + i) * k for i in range(5)]
    assert (dev.circuit_size(), dev.num_variables()) == (state[0] + 10 * (g + 1), state[1] + 10 * k)
    assert dev.check() == -1
    dev.close()


@pytest.mark.parametrize("strict", (False, True), ids=("le", "lt"))
def test_is_less_equal_each_under_a_lagging_stream(engine, strict):
    """a composer made on the default stream; the two arrays of Variables are filled in on a side stream that is behind: while the
    host issues the call they hold other Variables"""
    num_bits, batch = 16, 40
    rng = random.Random(79)
    side = torch.cuda.Stream()
    values = pairs_of_values(num_bits, batch, rng)
    comp = pg.StandardComposer(engine, 1 << 12, 1 << 13)
    first = comp.add_input_batch(dev_scalars([x for x, _ in values] + [y for _, y in values]))
    mod = model_of(comp)
    n0, nv0 = comp.circuit_size(), comp.num_variables()
    xs, ys = list(range(first, first + batch)), list(range(first + batch, first + 2 * batch))
    t_x, t_y = tv(xs), tv(ys)
    xv, yv = tv(ys[::-1]), tv(xs[::-1])     # stale: other Variables
    c0 = pg.StandardComposer(engine, 1 << 12, 1 << 13)  # warm-up on another composer, under both streams
    c0.add_input_batch(dev_scalars([x for x, _ in values] + [y for _, y in values]))
    c0.is_less_equal_each(xv, yv, num_bits, strict)
    with torch.cuda.stream(side):
        c0.is_less_equal_each(xv, yv, num_bits, strict)
    c0.sync()
    c0.close()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            ev = lagging(side)
            xv.copy_(t_x)
            yv.copy_(t_y)
            assert not ev.query(), LATE
            res = comp.is_less_equal_each(xv, yv, num_bits, strict)  # (it checks its arrays first: a host synchronisation)
            got_check = comp.check()
        torch.cuda.synchronize()
        exp = [mod.is_less_equal(x, y, num_bits, strict)[1] for x, y in zip(xs, ys)]
        assert res.cpu().tolist() == exp
        assert [mod.values[r] for r in exp] == [int(x < y if strict else x <= y) for x, y in values]
        compare(comp, mod, n0, nv0)
        assert got_check == -1 and mod.first_bad() == -1
        assert_q_range(comp, mod)
    finally:
        release()
        comp.close()
