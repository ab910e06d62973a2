"""CPU: the replay of is_less_equal on the C oracle's composer (tests/compare_gate_oracle.py) against the Python-integer model
(tests/compare_gate_model.py): rows, selectors, new Variables, the q_range rows and the first failing row, for every width and both
`strict` values.  Then sigma of circuits with compare rows: its cycles are exactly the positions of each Variable -- x and y in the
terminal rows among them, and one cycle through both where x and y are the same Variable."""
import random

import pytest

from oracle import pyoracle as po
from tests import compare_gate_model as cm
from tests import compare_gate_oracle as co
from tests import interval_gate_model as im
from tests import test_widget_oracle as two
from tests import widget_oracle as wo

R = cm.R


def model_of(ora):
    vals = [wo.int_of(l) for l in ora.export()["var_values"]]
    return cm.Circuit(n_rows=ora.n, values=vals, zero_var=int(ora.L.composer_zero_var(ora.c)))


def directed(num_bits):
    top = 2**num_bits - 1
    mid = 2**(num_bits - 1) + 1
    return [(mid, mid), (mid, mid + 1), (mid + 1, mid), (0, top), (top, 0), (0, 0), (0, 3 * 2**num_bits + 1), (R - 1, 0)]


@pytest.mark.parametrize("strict", (False, True))
@pytest.mark.parametrize("num_bits", cm.NUM_BITS)
def test_replay_equals_the_model(num_bits, strict):
    k, g, pad = cm.layout(num_bits)
    rnd = random.Random(num_bits * 2 + strict)
    for x, y in directed(num_bits) + [(rnd.randrange(2**num_bits), rnd.randrange(2**num_bits))]:
        ora, wid = po.Composer(), co.CompareWidgets()
        mod = model_of(ora)
        xv, yv = two.add_input(ora, mod, x), two.add_input(ora, mod, y)
        n0 = ora.n
        got = wid.is_less_equal(ora, xv, yv, num_bits, strict)
        assert got == mod.is_less_equal(xv, yv, num_bits, strict) == (n0, yv + 1)
        assert ora.n == n0 + cm.rows_per_item(num_bits) and ora.num_vars == yv + 1 + cm.vars_per_item(num_bits)
        two.compare(ora, wid, mod, n0)
        assert wid.q_range_rows == list(range(n0, n0 + g))
        # the link on the terminal row holds whatever the witnesses: z is computed from them
        exp = ora.export()
        sel = tuple(wo.int_of(exp[s][n0 + g]) for s in two.SELECTORS)
        assert sel == (0, 1, R - 1, 1, (strict - 2**num_bits) % R)
        assert (int(exp["w_l"][n0 + g]), int(exp["w_r"][n0 + g]), int(exp["w_o"][n0 + g])) == (yv + k, yv, xv)
        assert im.arith_holds(sel, *(mod.values[v] for v in mod.rows[n0 + g]))
        assert ora.check() == -1
        bad = wid.first_bad(ora)
        assert bad == mod.first_bad()
        if x < 2**num_bits and y < 2**num_bits:
            assert bad == -1 and mod.values[got[1]] == int(x < y if strict else x <= y)
        elif y == 3 * 2**num_bits + 1:       # c(z) = 2^K + 1 - strict does not fit the widget: the item's row 0
            assert bad == n0
        # a batch behind it: the same pair again, swapped, the same Variable on both sides, zero_var on either side
        res = wid.is_less_equal_each(ora, [xv, yv, xv, 0, yv], [yv, xv, xv, yv, 0], num_bits, strict)
        exp_res = [mod.is_less_equal(a, b, num_bits, strict)[1] for a, b in ((xv, yv), (yv, xv), (xv, xv), (0, yv), (yv, 0))]
        assert res == exp_res
        two.compare(ora, wid, mod, n0)
        assert wid.first_bad(ora) == mod.first_bad()
        assert mod.values[res[2]] == int(not strict)        # x against itself, whatever x holds


def test_sigma_cycles_are_the_variables_positions():
    rnd = random.Random(23)
    ora, wid = po.Composer(), co.CompareWidgets()
    ws = [ora.add_input(po.limbs(wo.fr_of(v))) for v in (rnd.randrange(2**8), 255, 3, rnd.randrange(2**8))]
    wid.range_gate_batch(ora, ws, 8)
    s = int(ora.L.composer_add(ora.c, wo.fr_of(1), ws[1], wo.fr_of(1), ws[2], wo.fr_of(0), None))       # the result of a gate as y
    res = wid.is_less_equal_each(ora, [ws[0], ws[0], ws[1], 0, ws[3]], [ws[3], ws[0], s, ws[2], 0], 8)   # x is y; zero_var as x, as y
    bit = wid.is_less_equal(ora, ws[2], ws[1], 62, True)[1]
    ora.L.conditionally_select_zero(ora.c, ws[0], res[0])          # the results go on as wires of other rows
    ora.L.composer_constrain_to_constant(ora.c, bit, wo.fr_of(1), None)
    wid.is_less_equal(ora, res[1], bit, 2)                         # ... and as inputs of another comparison (k = 2, g = 1)
    n = ora.n
    for padded in (n, 1 << (n - 1).bit_length()):
        by_var = two.check_sigma(ora, padded)
    exp = ora.export()
    terminal = [i + 1 for i in wid.q_range_rows if i + 1 not in wid.q_range_rows]
    compare_rows = [i for i in terminal if wo.int_of(exp["q_l"][i]) == 1]
    assert len(compare_rows) == 7
    # ws[0]: its range item's terminal row; x of item 0; x AND y of item 1 (two positions of one row); select_zero's input
    t1 = compare_rows[1]
    assert {1 * padded + t1, 2 * padded + t1} <= set(by_var[ws[0]])
    assert sum(1 for p in by_var[ws[0]] if p % padded in compare_rows) == 3
    # zero_var sits on w_o of item 3's terminal row (x) and on w_r of item 4's (y)
    assert 2 * padded + compare_rows[3] in by_var[0] and 1 * padded + compare_rows[4] in by_var[0]
    # a result: its own widget's positions, and those of the rows that use it
    assert len(by_var[res[0]]) > 1 and len(by_var[bit]) >= 3
    assert wid.first_bad(ora) == -1
