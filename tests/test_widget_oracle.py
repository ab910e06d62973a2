"""CPU: the replay of range_gate / interval_gate on the C oracle's composer (tests/widget_oracle.py) against the two Python-integer
models, for every width of their NUM_BITS and their edge values: rows, new Variables, the q_range bitmap, the first failing row,
the arithmetic statement of every row.  Then sigma of circuits with widget rows, checked in plain Python without the oracle's C
bookkeeping: a permutation whose cycles are exactly the sets of positions that hold one Variable -- the property the GPU tests
inherit when they find the device's sigma limb-equal to this one."""
import random

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import interval_gate_model as im
from tests import range_gate_model as m
from tests import widget_oracle as wo

R = m.R
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c")


def model_of(ora):
    vals = [wo.int_of(l) for l in ora.export()["var_values"]]
    return im.Circuit(n_rows=ora.n, values=vals, zero_var=int(ora.L.composer_zero_var(ora.c)))


def add_input(ora, mod, v):
    var = ora.add_input(po.limbs(wo.fr_of(v)))
    assert var == mod.add_input(v)
    return var


def compare(ora, wid, mod, n0):
    """rows n0.. of the oracle == the model's: wires, selectors, q_range; every Variable's value; w_4 = zero_var"""
    exp = ora.export()
    assert ora.n == len(mod.rows) and ora.num_vars == len(mod.values)
    assert [wo.int_of(l) for l in exp["var_values"]] == mod.values
    for j, k in enumerate(("w_l", "w_r", "w_o")):
        assert exp[k][n0:].tolist() == [r[j] for r in mod.rows[n0:]], k
    for j, k in enumerate(SELECTORS):
        assert [wo.int_of(l) for l in exp[k][n0:]] == [s[j] for s in mod.sel[n0:]], k
    full = ora.full_columns()
    assert not full["w_4"][n0:].any() and not full["q_4"][n0:].any() and mod.zero_var == 0
    col = wid.q_range_column(ora)
    assert col.shape == (ora.n, 4)
    assert [bool(r.any()) for r in col] == [bool(q) for q in mod.q_range]
    assert all(np.array_equal(r, wo.ONE) for r in col[np.array(mod.q_range, dtype=bool)])


@pytest.mark.parametrize("num_bits", m.NUM_BITS)
def test_range_gate_replay_equals_the_model(num_bits):
    rnd = random.Random(num_bits)
    for v in list(m.edge_values(num_bits)) + [rnd.randrange(2**num_bits), rnd.randrange(R)]:
        ora, wid = po.Composer(), wo.Widgets()
        mod = model_of(ora)
        w = add_input(ora, mod, v)
        n0 = ora.n
        assert wid.range_gate(ora, w, num_bits) == n0 == mod.range_gate(w, num_bits)
        assert ora.n == n0 + m.rows_per_item(num_bits) and ora.num_vars == w + 1 + m.vars_per_item(num_bits)
        compare(ora, wid, mod, n0)
        assert ora.check() == -1       # no arithmetic on a range item
        assert wid.first_bad(ora) == mod.first_bad() == (-1 if v < 2**num_bits else n0)
        # a second item on the same witness and one on zero_var, behind it
        wid.range_gate_batch(ora, [w, 0], num_bits)
        mod.range_gate(w, num_bits)
        mod.range_gate(0, num_bits)
        compare(ora, wid, mod, n0)
        assert wid.first_bad(ora) == mod.first_bad()


@pytest.mark.parametrize("num_bits", im.NUM_BITS)
def test_interval_gate_replay_equals_the_model(num_bits):
    k, g, pad = im.layout(num_bits)
    for lo, hi in im.edge_cases(num_bits):
        for v in im.edge_witnesses(lo, hi):
            ora, wid = po.Composer(), wo.Widgets()
            mod = model_of(ora)
            w = add_input(ora, mod, v)
            n0 = ora.n
            assert wid.interval_gate(ora, w, lo, hi, num_bits) == n0 == mod.interval_gate(w, lo, hi, num_bits)
            assert ora.n == n0 + im.rows_per_item(num_bits) and ora.num_vars == w + 1 + im.vars_per_item(num_bits)
            compare(ora, wid, mod, n0)
            # the subtractions on the terminal rows hold whatever the witness: d is computed from it
            exp = ora.export()
            vals = mod.values
            for i in range(n0, ora.n):
                sel = tuple(wo.int_of(exp[s][i]) for s in SELECTORS)
                assert im.arith_holds(sel, vals[exp["w_l"][i]], vals[exp["w_r"][i]], vals[exp["w_o"][i]]), i
            for h, q_r, q_c in ((0, R - 1, lo % R), (1, 1, -hi % R)):
                i = n0 + h * (g + 1) + g
                assert tuple(wo.int_of(exp[s][i]) for s in SELECTORS) == (0, 1, q_r, 0, q_c)
                assert (int(exp["w_r"][i]), int(exp["w_o"][i])) == (w, 0) and not wid.q_range_column(ora)[i].any()
            assert ora.check() == -1
            bad = wid.first_bad(ora)
            assert bad == mod.first_bad()
            assert (bad == -1) == (lo <= v <= hi), (lo, hi, v, bad)


def test_batches_are_loops_in_item_order():
    rnd = random.Random(3)
    ora, wid = po.Composer(), wo.Widgets()
    mod = model_of(ora)
    ws = [add_input(ora, mod, rnd.randrange(2**16)) for _ in range(6)]
    n0 = ora.n
    wid.range_gate_batch(ora, ws[:3], 16)
    wid.interval_gate_batch(ora, ws[1:4], 0, 2**16 - 1, 16)
    los = [0, 5, R - 2**16]
    his = [2**16 - 1, 5 + 2**16 - 1, R - 1]
    wid.interval_gate_ragged_batch(ora, ws[3:], los, his, 16)
    for w in ws[:3]:
        mod.range_gate(w, 16)
    for w in ws[1:4]:
        mod.interval_gate(w, 0, 2**16 - 1, 16)
    for w, lo, hi in zip(ws[3:], los, his):
        mod.interval_gate(w, lo, hi, 16)
    compare(ora, wid, mod, n0)
    assert wid.first_bad(ora) == mod.first_bad()


def test_first_bad_is_the_minimum_of_both_statements():
    """an arithmetic failure in front of a failing widget row, and behind it"""
    for ctc_first in (True, False):
        ora, wid = po.Composer(), wo.Widgets()
        w = ora.add_input(po.limbs(wo.fr_of(2**16)))
        rows = []
        for step in ((0, 1) if ctc_first else (1, 0)):
            rows.append(ora.n)
            if step == 0:
                ora.L.composer_constrain_to_constant(ora.c, w, wo.fr_of(5), None)
            else:
                wid.range_gate(ora, w, 16)
        assert wid.first_bad(ora) == rows[0] == 3
        assert ora.check() == rows[0 if ctc_first else 1]
        assert wid.first_q_range_bad(ora) == rows[1 if ctc_first else 0]


def positions_by_variable(ora, padded):
    exp, n = ora.export(), ora.n
    wires = [exp["w_l"], exp["w_r"], exp["w_o"], ora.full_columns()["w_4"]]
    by_var = {}
    for g in range(n):          # recording order: gate by gate, wire by wire
        for w in range(4):
            by_var.setdefault(int(wires[w][g]), []).append(w * padded + g)
    return by_var


def check_sigma(ora, padded):
    """sigma is a permutation of the 4 * padded positions (position = wire * padded + gate); the cycle through a Variable's first
    position is the list of ALL its positions in recording order, each mapped to the next; padding rows map to themselves"""
    n = ora.n
    sig = ora.sigma(padded).reshape(-1).tolist()
    assert sorted(sig) == list(range(4 * padded))
    by_var = positions_by_variable(ora, padded)
    assert sum(len(p) for p in by_var.values()) == 4 * n
    for var, pos in by_var.items():
        for here, there in zip(pos, pos[1:] + pos[:1]):
            assert sig[here] == there, (var, here, sig[here], there)
    for w in range(4):
        for g in range(n, padded):
            assert sig[w * padded + g] == w * padded + g
    return by_var


def test_sigma_cycles_are_the_variables_positions():
    rnd = random.Random(11)
    ora, wid = po.Composer(), wo.Widgets()
    ws = [ora.add_input(po.limbs(wo.fr_of(v))) for v in (rnd.randrange(2**8), 255, 3, rnd.randrange(2**8), 1)]
    wid.range_gate_batch(ora, [ws[0], ws[0], ws[1], 0], 8)             # a repeated witness, zero_var as a witness
    prod = int(ora.L.composer_mul(ora.c, wo.fr_of(1), ws[1], ws[2], wo.fr_of(0), None))
    wid.interval_gate_batch(ora, [ws[0], ws[3]], 0, 255, 8)
    wid.range_gate(ora, prod, 16)                                     # the result of a gate as a witness
    ora.L.composer_constrain_to_constant(ora.c, ws[4], wo.fr_of(1), None)
    wid.interval_gate_ragged_batch(ora, [ws[4], ws[4]], [0, 1], [3, 1 + 63], 6)
    wid.range_gate(ora, ws[2], 2)                                     # k = 1: no new Variable, pad = 2
    n = ora.n
    for padded in (n, 1 << (n - 1).bit_length()):
        by_var = check_sigma(ora, padded)
    # what the widget rows add to zero_var's cycle: the pad positions, the two idle wires of a range item's terminal row, w_o of
    # an interval half's, and w_4 of every row
    rows = widget_rows(wid)
    assert sum(1 for p in by_var[0] if p % padded in rows) > len(rows)   # more than the w_4 position a row
    # ws[0] is the witness of two range items and of one interval: a terminal position each, two for the interval
    assert len(by_var[ws[0]]) == 4
    assert wid.first_bad(ora) == -1


def widget_rows(wid):
    """the q_range rows and the terminal rows behind each run of them"""
    rows = set(wid.q_range_rows)
    return rows | {i + 1 for i in rows if i + 1 not in rows}
