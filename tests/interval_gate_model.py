"""A model of interval_gate(witness, min, max, num_bits) in Python integers, independent of the library: two
range widgets (tests/range_gate_model.py) on d = witness - min (half 0) and d = max - witness (half 1), whose terminal rows carry
the subtractions.

k, g, pad as in range_gate_model.  An item owns 2 (g + 1) rows and 2 k new Variables; half h takes rows h (g + 1) .. and
Variables first + h k ..: k - 1 accumulators of d's canonical integer, then d itself, which is the widget's P(3g).
  row i < g of the half: the widget's, q_range = 1, arithmetic selectors 0
  row g of the half:     (d, witness, zero_var), q_range = 0, q_l = 1 and (q_r, q_c) = (-1, +min) for h = 0, (+1, -max) for h = 1
Preconditions: num_bits even in [2, 252], min <= max and max - min < 2^num_bits as integers below r."""
from tests import range_gate_model as m

R = m.R

NUM_BITS = (2, 4, 6, 8, 62, 64, 252)   # pad = 2, 1, 0 with g = 1 and with g > 1


def layout(num_bits):
    """(k, g, pad); ValueError for what the library refuses"""
    if num_bits > 252:
        raise ValueError(f"num_bits = {num_bits}")
    return m.layout(num_bits)


def check_bounds(lo, hi, num_bits):
    layout(num_bits)
    if not (0 <= lo <= hi < R) or hi - lo >= 2**num_bits:
        raise ValueError(f"bounds {lo}, {hi} at {num_bits} bits")


def rows_per_item(num_bits):
    return 2 * (layout(num_bits)[1] + 1)


def vars_per_item(num_bits):
    return 2 * layout(num_bits)[0]


def item(witness_var, value, lo, hi, num_bits, first_var, zero_var, checked=True):
    """-> (rows, selectors, q_range, new_values): rows = [(a, b, c)] Variables, selectors = [(q_m, q_l, q_r, q_o, q_c)] integers
    below r, q_range = [0 or 1], new_values = the canonical integers of the 2 k Variables first_var .. the item creates.
    checked=False lays the item out for bounds that violate the width precondition (to show what the precondition is for)."""
    if checked:
        check_bounds(lo, hi, num_bits)
    k, g, pad = layout(num_bits)
    v = value % R
    rows, sel, qr, new = [], [], [], []
    for h, d, q_r, q_c in ((0, (v - lo) % R, R - 1, lo % R), (1, (hi - v) % R, 1, (-hi) % R)):
        d_var = first_var + h * k + (k - 1)
        w_rows, w_qr, accs = m.item(d_var, d, num_bits, first_var + h * k, zero_var)
        assert w_rows[g] == (d_var, zero_var, zero_var)
        rows += w_rows[:g] + [(d_var, witness_var, zero_var)]
        sel += [(0, 0, 0, 0, 0)] * g + [(0, 1, q_r, 0, q_c)]
        qr += w_qr
        new += accs + [d]
    assert len(rows) == 2 * (g + 1) and len(new) == 2 * k
    return rows, sel, qr, new


def arith_holds(sel, a, b, c):
    q_m, q_l, q_r, q_o, q_c = sel
    return (q_m * a * b + q_l * a + q_r * b + q_o * c + q_c) % R == 0


class Circuit(m.Circuit):
    """range_gate_model.Circuit with interval items: the selectors of the rows it models, and their arithmetic statement"""

    def __init__(self, n_rows=0, values=None, zero_var=0):
        super().__init__(n_rows, values, zero_var)
        self.sel = [None] * n_rows

    def range_gate(self, witness_var, num_bits):
        first = super().range_gate(witness_var, num_bits)
        self.sel += [(0, 0, 0, 0, 0)] * (len(self.rows) - first)
        return first

    def interval_gate(self, witness_var, lo, hi, num_bits, checked=True):
        rows, sel, qr, new = item(witness_var, self.values[witness_var], lo, hi, num_bits, len(self.values), self.zero_var, checked)
        first = len(self.rows)
        self.rows += rows
        self.sel += sel
        self.q_range += qr
        self.values += new
        return first

    def first_bad(self):
        """the first modelled row whose statement fails -- the widget's where q_range = 1, the arithmetic gate's everywhere --
        or -1"""
        for i, r in enumerate(self.rows):
            if r is None:
                continue
            a, b, c = (self.values[x] for x in r)
            if self.q_range[i] and not m.row_holds(a, b, c, self.values[self.rows[i + 1][0]]):
                return i
            if not arith_holds(self.sel[i], a, b, c):
                return i
        return -1


def edge_cases(num_bits):
    """(lo, hi) pairs: lo = 0, lo = hi, the widest legal interval, bounds that end at r - 1"""
    w = 2**num_bits - 1
    out = [(0, min(w, 1000)), (5, 5), (0, 0), (7, 7 + w), (0, w), (R - 1 - w, R - 1), (R - 1, R - 1), (R - 3, R - 1)]
    return [(lo, hi) for lo, hi in out if 0 <= lo <= hi < R and hi - lo <= w]


def edge_witnesses(lo, hi):
    return sorted({lo, hi, (lo - 1) % R, (hi + 1) % R, 0, R - 1, (lo + hi) // 2})
