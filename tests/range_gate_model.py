"""A model of range_gate(witness, num_bits) in Python integers: the quad-accumulator widget on three wires (DESIGN section
3.19), independent of the library.

k = num_bits / 2 quads, g = ceil(k / 3) widget rows, pad = 3g - k.  Positions p = 0 .. 3g of an item:
  P(p) = zero_var                                                      p <= pad
  P(p) = first_var + (p - pad - 1), value floor(v / 4^(3g - p)) mod r  pad < p < 3g
  P(3g) = the witness Variable
row i < g = (P(3i), P(3i+1), P(3i+2)) with q_range = 1; row g = (P(3g), zero_var, zero_var) with q_range = 0; the five
arithmetic selectors are 0 on every row.  A q_range row states that b - 4a, c - 4b and a_next - 4c lie in {0, 1, 2, 3}."""

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001

NUM_BITS = (2, 4, 6, 8, 60, 62, 64, 254)   # pad = 2, 1, 0 with g = 1 and with g > 1


def edge_values(num_bits):
    return (0, 2**num_bits - 1, 2**num_bits, R - 1)


def layout(num_bits):
    """(k, g, pad); ValueError for what the library refuses"""
    if num_bits < 2 or num_bits > 254 or num_bits % 2:
        raise ValueError(f"num_bits = {num_bits}")
    k = num_bits // 2
    g = (k + 2) // 3
    return k, g, 3 * g - k


def rows_per_item(num_bits):
    return layout(num_bits)[1] + 1


def vars_per_item(num_bits):
    return layout(num_bits)[0] - 1


def item(witness_var, value, num_bits, first_var, zero_var):
    """-> (rows, q_range, new_values): rows = [(a, b, c)] Variables, q_range = [0 or 1] per row, new_values = the canonical
    integers of the k - 1 Variables first_var .. the item creates"""
    k, g, pad = layout(num_bits)
    v = value % R

    def P(p):
        if p <= pad:
            return zero_var
        return first_var + (p - pad - 1) if p < 3 * g else witness_var
    rows = [(P(3 * i), P(3 * i + 1), P(3 * i + 2)) for i in range(g)] + [(P(3 * g), zero_var, zero_var)]
    new_values = [(v >> (2 * (3 * g - p))) % R for p in range(pad + 1, 3 * g)]
    assert len(new_values) == k - 1
    return rows, [1] * g + [0], new_values


def quad(f):
    return f % R in (0, 1, 2, 3)


def row_holds(a, b, c, a_next):
    """the statement of a q_range = 1 row over the VALUES of its wires and of the next row's first wire"""
    return quad(b - 4 * a) and quad(c - 4 * b) and quad(a_next - 4 * c)


def first_failing_row(rows, q_range, values):
    """index of the first q_range row whose statement fails (values: Variable -> integer), or -1"""
    for i, (a, b, c) in enumerate(rows):
        if q_range[i] and not row_holds(values[a], values[b], values[c], values[rows[i + 1][0]]):
            return i
    return -1


class Circuit:
    """a composer of range items only, enough to lay batches out as the library does: Variable 0 = zero_var = 0"""

    def __init__(self, n_rows=0, values=None, zero_var=0):
        self.values = list(values) if values is not None else [0]
        self.zero_var = zero_var
        self.rows = [None] * n_rows       # rows of other calls: not modelled
        self.q_range = [0] * n_rows

    def add_input(self, v):
        self.values.append(v % R)
        return len(self.values) - 1

    def range_gate(self, witness_var, num_bits):
        rows, qr, new = item(witness_var, self.values[witness_var], num_bits, len(self.values), self.zero_var)
        first = len(self.rows)
        self.rows += rows
        self.q_range += qr
        self.values += new
        return first

    def first_bad(self):
        for i, r in enumerate(self.rows):
            if self.q_range[i] and not row_holds(*(self.values[x] for x in r), self.values[self.rows[i + 1][0]]):
                return i
        return -1
