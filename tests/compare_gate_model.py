"""A model of is_less_equal(x, y, num_bits, strict) in Python integers, independent of the library: ONE range
widget (tests/range_gate_model.py) over K = num_bits + 2 bits on z = 2^num_bits + y - x - s (s = 1 if strict else 0), whose terminal
row carries the link between z and the two witnesses.

k = K / 2, g = ceil(k / 3), pad = 3g - k: range_gate_model.layout(K).  An item owns g + 1 rows and k new Variables first + kk,
kk = 0 .. k - 1, holding c(z) >> 2 (k - 1 - kk) for c(z) the canonical integer of z: `first` is the top quad -- the RESULT --,
first + k - 1 is z itself, the widget's P(3g).
  row i < g: the widget's, q_range = 1, arithmetic selectors 0
  row g:     (z, y, x), q_range = 0, q_l = 1, q_r = -1, q_o = +1, q_c = -2^num_bits + s   (z - y + x - 2^num_bits + s = 0)
The meaning of the result -- [x <= y], or [x < y] when strict -- has a PRECONDITION the gadget does not enforce: x, y < 2^num_bits."""
from tests import interval_gate_model as im
from tests import range_gate_model as m

R = m.R

NUM_BITS = (2, 4, 6, 62, 64, 252)   # k = 2, 3, 4, 32, 33, 127: pad = 1, 0, 2, 1, 0, 2 with g = 1 and with g > 1


def layout(num_bits):
    """(k, g, pad); ValueError for what the library refuses"""
    if num_bits < 2 or num_bits > 252 or num_bits % 2:
        raise ValueError(f"num_bits = {num_bits}")
    return m.layout(num_bits + 2)


def rows_per_item(num_bits):
    return layout(num_bits)[1] + 1


def vars_per_item(num_bits):
    return layout(num_bits)[0]


def item(x_var, y_var, x_value, y_value, num_bits, strict, first_var, zero_var):
    """-> (rows, selectors, q_range, new_values, result): rows = [(a, b, c)] Variables, selectors = [(q_m, q_l, q_r, q_o, q_c)]
    integers below r, q_range = [0 or 1], new_values = the canonical integers of the k Variables first_var .. the item creates,
    result = the Variable that holds the bit"""
    k, g, pad = layout(num_bits)
    s = 1 if strict else 0
    z = (2**num_bits + y_value - x_value - s) % R
    z_var = first_var + k - 1
    w_rows, w_qr, accs = m.item(z_var, z, num_bits + 2, first_var, zero_var)
    assert w_rows[g] == (z_var, zero_var, zero_var)
    rows = w_rows[:g] + [(z_var, y_var, x_var)]
    sel = [(0, 0, 0, 0, 0)] * g + [(0, 1, R - 1, 1, (s - 2**num_bits) % R)]
    new = accs + [z]
    assert len(rows) == g + 1 and len(new) == k
    return rows, sel, w_qr, new, first_var


class Circuit(im.Circuit):
    """interval_gate_model.Circuit (range and interval items, selectors, the arithmetic statement) with compare items"""

    def is_less_equal(self, x_var, y_var, num_bits, strict=False):
        """-> (the item's first row, the result Variable)"""
        rows, sel, qr, new, result = item(x_var, y_var, self.values[x_var], self.values[y_var], num_bits, strict, len(self.values),
                                          self.zero_var)
        first = len(self.rows)
        self.rows += rows
        self.sel += sel
        self.q_range += qr
        self.values += new
        return first, result
