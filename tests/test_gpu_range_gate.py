"""GPU: range_gate / range_gate_batch on the device composer against the Python-integer model (tests/range_gate_model.py):
every limb of the rows, wires and new Variables, materialize's q_range column, check() and the copy constraints, for every
pad (2, 1, 0) with one and with several widget rows and batches that stay inside and cross an emitter workgroup (256 items)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import _lib, synth
from tests import range_gate_model as m

pytestmark = pytest.mark.gpu

S = pg.BlsScalar.from_int
ONE = np.array(synth.mont(1), dtype=np.uint64)


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def dev_scalars(vals):
    return torch.from_numpy(synth.scalars_from_ints(vals).view(np.int64)).cuda()


def tv(xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.int64, device="cuda")


def u64(a):
    return np.ascontiguousarray(np.asarray(a)).view(np.uint64)


def witnesses(dev, values):
    """Variables holding `values`, from two earlier calls: the even ones of an add_input_batch, the odd ones the results of a
    mul_batch (inputs times a Variable that holds 1)"""
    ev, od = list(values[0::2]), list(values[1::2])
    first = dev.add_input_batch(dev_scalars(ev))
    out = [0] * len(values)
    out[0::2] = range(first, first + len(ev))
    if od:
        one = dev.add_input(S(1))
        src = dev.add_input_batch(dev_scalars(od))
        res = dev.mul_batch(S(1), tv(range(src, src + len(od))), tv([one] * len(od)), S(0))
        out[1::2] = res.cpu().tolist()
    return out


def model_of(dev):
    """the model circuit behind the composer as it stands (rows of other calls are not modelled)"""
    vals = [synth.to_int(l) for l in u64(dev.export()["var_values"])]
    return m.Circuit(n_rows=dev.circuit_size(), values=vals, zero_var=dev.zero_var)


def in_range_values(num_bits, n, rnd):
    """n values below 2^num_bits with both ends of the range among them"""
    if n == 1:
        return [2**num_bits - 1]
    vals = [0, 2**num_bits - 1] + [rnd.randrange(2**num_bits) for _ in range(n - 2)]
    rnd.shuffle(vals)
    return vals


def compare(dev, mod, n0, nv0):
    got = dev.export(n0, nv0)
    rows = mod.rows[n0:]
    assert dev.circuit_size() == len(mod.rows) and dev.num_variables() == len(mod.values)
    for k in ("q_m", "q_l", "q_r", "q_o", "q_c"):
        assert not u64(got[k]).any(), k
    for j, k in enumerate(("w_l", "w_r", "w_o")):
        assert np.array_equal(u64(got[k]), np.array([r[j] for r in rows], dtype=np.uint64)), k
    assert np.array_equal(u64(got["var_values"]).reshape(-1, 4), synth.scalars_from_ints(mod.values[nv0:])), "var_values"


def q_range_expected(mod):
    exp = np.zeros((len(mod.rows), 4), dtype=np.uint64)
    exp[np.array(mod.q_range, dtype=bool)] = ONE
    return exp


@pytest.mark.parametrize("batch", (1, 3, 257))
@pytest.mark.parametrize("num_bits", m.NUM_BITS)
def test_emission_materialize_and_check(engine, num_bits, batch):
    rnd = random.Random(num_bits * 1000 + batch)
    k, g, pad = m.layout(num_bits)
    dev = pg.StandardComposer(engine, gate_capacity=1 << 15, var_capacity=1 << 17)
    good = in_range_values(num_bits, batch, rnd)
    bad = in_range_values(num_bits, batch, rnd)
    first_bad_item = batch // 2
    bad[first_bad_item] = 2**num_bits
    bad[-1] = m.R - 1 if batch > 1 else 2**num_bits
    wv = witnesses(dev, good + bad)
    mod = model_of(dev)
    n0, nv0 = dev.circuit_size(), dev.num_variables()

    # every witness in range
    dev.range_gate_batch(tv(wv[:batch]), num_bits)
    for w in wv[:batch]:
        mod.range_gate(w, num_bits)
    compare(dev, mod, n0, nv0)
    assert dev.circuit_size() == n0 + batch * (g + 1) and dev.num_variables() == nv0 + batch * (k - 1)
    assert dev.check() == -1 and mod.first_bad() == -1
    assert dev.copy_constraints_hold()

    # q_range alone (every other pointer NULL) and with all columns
    alone = torch.full((dev.circuit_size() + 1, 4), -1, dtype=torch.int64, device="cuda")  # (a sentinel row behind it)
    st = dev._lib.pg_composer_materialize(dev._h, C.byref(_lib.FullColumnsC(q_range=alone.data_ptr())))
    assert st == 0
    assert np.array_equal(u64(alone[:-1].cpu().numpy()), q_range_expected(mod))
    assert (alone[-1] == -1).all()
    full = dev.materialize()
    assert np.array_equal(u64(full["q_range"].cpu().numpy()), q_range_expected(mod))
    assert (u64(full["q_arith"].cpu().numpy()) == ONE).all()
    for name in ("q_logic", "q_fixed_group_add", "q_variable_group_add"):
        assert not full[name].any()
    vals = np.array([synth.mont(v) for v in mod.values], dtype=np.uint64)
    for j, name in enumerate(("w_l_value", "w_r_value", "w_o_value")):
        exp = vals[np.array([r[j] for r in mod.rows[n0:]], dtype=np.int64)]
        assert np.array_equal(u64(full[name][n0:].cpu().numpy()), exp), name

    # one accumulator overwritten through the composer's own columns names its row
    if k > 1:
        j = rnd.randrange(batch * (k - 1))
        cols = dev.device_columns()
        keep = cols.var_values[nv0 + j].clone()
        cols.var_values[nv0 + j] = dev_scalars([mod.values[nv0 + j] + 5])[0]
        changed = m.Circuit(values=mod.values, zero_var=mod.zero_var)
        changed.rows, changed.q_range = mod.rows, mod.q_range
        changed.values[nv0 + j] += 5
        assert changed.first_bad() >= n0
        assert dev.check() == changed.first_bad()
        cols.var_values[nv0 + j] = keep
        del cols
        assert dev.check() == -1

    # a second call right behind the first (one segment), with witnesses out of range: all their rows, row 0 of the first one fails
    n1, nv1 = dev.circuit_size(), dev.num_variables()
    dev.range_gate_batch(tv(wv[batch:]), num_bits)
    for w in wv[batch:]:
        mod.range_gate(w, num_bits)
    compare(dev, mod, n1, nv1)
    assert mod.first_bad() == n1 + first_bad_item * (g + 1)
    assert dev.check() == mod.first_bad()
    assert dev.copy_constraints_hold()
    assert np.array_equal(u64(dev.materialize()["q_range"].cpu().numpy()), q_range_expected(mod))
    dev.close()


def test_single_calls_and_mixed_bounds(engine):
    """the single call on Variables of single calls, bounds of different g one after the other (separate segments) with gate rows
    between them; an arithmetic failure before the range rows wins the minimum"""
    dev = pg.StandardComposer(engine)
    vals = {8: 200, 62: 2**62 - 1, 16: 65535, 2: 3, 254: 2**254 - 1}
    ws = {b: dev.add_input(S(v)) for b, v in vals.items()}
    mod = model_of(dev)
    n0, nv0 = dev.circuit_size(), dev.num_variables()
    for b in (8, 62):
        dev.range_gate(ws[b], b)
        mod.range_gate(ws[b], b)
    compare(dev, mod, n0, nv0)
    dev.constrain_to_constant(ws[8], S(200))
    mod.rows.append(None)
    mod.q_range.append(0)
    n1, nv1 = dev.circuit_size(), dev.num_variables()
    for b in (16, 2, 254):
        dev.range_gate(ws[b], b)
        mod.range_gate(ws[b], b)
    compare(dev, mod, n1, nv1)
    assert dev.check() == -1 and dev.copy_constraints_hold()
    assert np.array_equal(u64(dev.materialize()["q_range"].cpu().numpy()), q_range_expected(mod))
    # out of range by one
    w = dev.add_input(S(2**16))
    row = dev.circuit_size()
    dev.range_gate(w, 16)
    assert dev.check() == row
    dev.constrain_to_constant(ws[8], S(201))  # an arithmetic failure behind it: the range row is still the first
    assert dev.check() == row
    dev.close()
    dev = pg.StandardComposer(engine)
    w = dev.add_input(S(2**16))
    dev.constrain_to_constant(w, S(5))  # an arithmetic failure in front of it
    dev.range_gate(w, 16)
    assert dev.check() == 3
    dev.close()


def test_refused_calls_append_nothing(engine):
    dev = pg.StandardComposer(engine)
    first = dev.add_input_batch(dev_scalars([1, 2, 3]))
    state = (dev.circuit_size(), dev.num_variables())
    good = tv(range(first, first + 3))
    for bits in (0, 1, 7, 255, 256, 2**32 + 8):
        with pytest.raises(pg.PgError):
            dev.range_gate_batch(good, bits)
        with pytest.raises(pg.PgError):
            dev.range_gate(first, bits)
    nv = dev.num_variables()
    with pytest.raises(pg.PgError):
        dev.range_gate_batch(tv([first, nv, first + 1]), 8)  # a Variable the composer does not have
    with pytest.raises(pg.PgError):
        dev.range_gate(nv, 8)
    lib = dev._lib
    assert lib.pg_composer_range_gate_batch(None, good.data_ptr(), 8, 3) == 2
    assert lib.pg_composer_range_gate_batch(dev._h, None, 8, 3) == 2
    assert lib.pg_composer_range_gate(None, 0, 8) == 2
    assert (dev.circuit_size(), dev.num_variables()) == state and dev.check() == -1
    assert not dev.materialize()["q_range"].any()
    dev.range_gate_batch(good[:0], 8)  # an empty batch is nothing
    assert (dev.circuit_size(), dev.num_variables()) == state
    dev.close()


def test_clear_witness_finds_the_rows_in_place(engine):
    """after clear_witness the same calls with other witnesses write assignments only (refresh_stats), and the composer equals
    a fresh build of the second witnesses"""
    rnd = random.Random(5)

    def program(dev, values):
        wv = witnesses(dev, values)
        dev.range_gate_batch(tv(wv[:300]), 62)
        dev.range_gate_batch(tv(wv[300:]), 8)
        dev.range_gate(wv[0], 64)
        dev.range_gate(wv[301], 2)
        return wv

    def values():
        return [rnd.randrange(2**62) for _ in range(300)] + [rnd.randrange(4)] * 2 + [rnd.randrange(256) for _ in range(3)]

    dev = pg.StandardComposer(engine)
    program(dev, values())
    n_rows = dev.circuit_size()
    assert dev.check() == -1
    dev.clear_witness()
    second = values()
    program(dev, second)
    kept, rewritten, refreshing = dev.refresh_stats()
    assert (kept, rewritten, refreshing) == (n_rows - 3, 0, True)
    fresh = pg.StandardComposer(engine)
    program(fresh, second)
    a, b = dev.export(), fresh.export()
    for k in a:
        assert np.array_equal(u64(a[k]), u64(b[k])), k
    assert dev.check() == -1 and dev.copy_constraints_hold()
    assert torch.equal(dev.materialize()["q_range"], fresh.materialize()["q_range"])
    # other witnesses, one of them out of range: its rows are still in place, and check names the item's first row
    dev.clear_witness()
    third = values()
    third[7] = 2**62
    program(dev, third)
    assert dev.refresh_stats() == (n_rows - 3, 0, True)
    n_mul = len(third) // 2
    assert dev.check() == 3 + n_mul + 7 * m.rows_per_item(62)
    dev.close()
    fresh.close()
