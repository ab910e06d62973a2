"""TEST INFRASTRUCTURE, CPU: range_gate and interval_gate (DESIGN sections 3.19, 3.20) replayed call for call on the C oracle's
composer (oracle.pyoracle.Composer), which has neither.  The layouts are those of tests/range_gate_model.py and
tests/interval_gate_model.py -- item() of either says which Variable sits on which wire and what the new Variables hold; this
module only records that through composer_add_input and composer_poly_gate (w_4 = zero_var, q_4 = 0), so that the oracle's own
bookkeeping gives the columns, check() and sigma of a circuit that mixes widget rows with everything else it knows.

An item is its new Variables first (k - 1 accumulators; 2 k for an interval, d among them), then its rows; a batch is a loop in
item order.  q_range is not a column of the oracle: the Widgets object keeps the rows that carry it."""
import numpy as np

from oracle import pyoracle as po
from oracle.model import MASK64, Q, R as MONT_R
from tests import interval_gate_model as im
from tests import range_gate_model as m

assert m.R == Q
R_INV = pow(MONT_R, -1, Q)
ONE = np.array(po.ints_to_mont_array([1])[0], dtype=np.uint64)


def fr_of(x):
    """canonical integer -> the oracle's Fr (Montgomery limbs from the big-integer model, not from fr.c)"""
    v = (x % Q) * MONT_R % Q
    f = po.Fr()
    f.l[0], f.l[1], f.l[2], f.l[3] = v & MASK64, (v >> 64) & MASK64, (v >> 128) & MASK64, v >> 192
    return f


def int_of(limbs):
    """Montgomery limbs (an Fr's, or a row of an exported array) -> canonical integer"""
    return (int(limbs[0]) | int(limbs[1]) << 64 | int(limbs[2]) << 128 | int(limbs[3]) << 192) * R_INV % Q


ZERO = fr_of(0)


class Widgets:
    """the widget appends on one oracle composer, and which of its rows carry q_range"""

    def __init__(self):
        self.q_range_rows = []     # ascending

    def _value(self, ora, var):
        return int_of(ora.L.composer_value(ora.c, int(var)).l)

    def _record(self, ora, rows, sel, q_range, new_values, first_var):
        for j, v in enumerate(new_values):
            assert ora.add_input(po.limbs(fr_of(v))) == first_var + j
        n0 = ora.n
        for (a, b, c), s in zip(rows, sel):
            ora.L.composer_poly_gate(ora.c, a, b, c, *[ZERO if x == 0 else fr_of(x) for x in s], None)
        self.q_range_rows += [n0 + i for i, q in enumerate(q_range) if q]
        return n0

    def range_gate(self, ora, witness_var, num_bits):
        """-> the item's first row"""
        first_var, zero = ora.num_vars, int(ora.L.composer_zero_var(ora.c))
        rows, qr, new = m.item(int(witness_var), self._value(ora, witness_var), num_bits, first_var, zero)
        return self._record(ora, rows, [(0, 0, 0, 0, 0)] * len(rows), qr, new, first_var)

    def interval_gate(self, ora, witness_var, lo, hi, num_bits):
        first_var, zero = ora.num_vars, int(ora.L.composer_zero_var(ora.c))
        rows, sel, qr, new = im.item(int(witness_var), self._value(ora, witness_var), lo, hi, num_bits, first_var, zero)
        return self._record(ora, rows, sel, qr, new, first_var)

    def range_gate_batch(self, ora, witness_vars, num_bits):
        for w in witness_vars:
            self.range_gate(ora, w, num_bits)

    def interval_gate_batch(self, ora, witness_vars, lo, hi, num_bits):
        for w in witness_vars:
            self.interval_gate(ora, w, lo, hi, num_bits)

    def interval_gate_ragged_batch(self, ora, witness_vars, los, his, num_bits):
        assert len(witness_vars) == len(los) == len(his)
        for w, lo, hi in zip(witness_vars, los, his):
            self.interval_gate(ora, w, lo, hi, num_bits)

    def first_q_range_bad(self, ora):
        """the first q_range row whose statement (range_gate_model.row_holds, Python integers) fails, or -1"""
        if not self.q_range_rows:
            return -1
        exp = ora.export()
        w_l, w_r, w_o, vals = exp["w_l"], exp["w_r"], exp["w_o"], exp["var_values"]
        seen = {}

        def val(var):
            var = int(var)
            if var not in seen:
                seen[var] = int_of(vals[var])
            return seen[var]
        for i in self.q_range_rows:
            if not m.row_holds(val(w_l[i]), val(w_r[i]), val(w_o[i]), val(w_l[i + 1])):
                return i
        return -1

    def first_bad(self, ora):
        """what the library's check() answers: the first row whose arithmetic gate or widget statement fails, or -1"""
        bad = [x for x in (ora.check(), self.first_q_range_bad(ora)) if x >= 0]
        return min(bad) if bad else -1

    def q_range_column(self, ora):
        """uint64[n, 4]: Montgomery one on the widget rows, zero elsewhere"""
        col = np.zeros((ora.n, 4), dtype=np.uint64)
        if self.q_range_rows:
            col[np.array(self.q_range_rows, dtype=np.int64)] = ONE
        return col
