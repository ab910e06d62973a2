"""CPU: the model of the three-wire range widget (tests/range_gate_model.py) against its specification in Python integers:
the layout for every pad and g, and "every widget row's statement holds iff v < 2^num_bits" on the edge values."""
import random

import pytest

from tests import range_gate_model as m

R = m.R


def test_layout_covers_every_pad_with_one_and_with_several_rows():
    seen = {(m.layout(b)[2], m.layout(b)[1] > 1) for b in m.NUM_BITS}
    assert seen == {(p, many) for p in (0, 1, 2) for many in (False, True)}
    assert [m.layout(b) for b in m.NUM_BITS] == [(1, 1, 2), (2, 1, 1), (3, 1, 0), (4, 2, 2), (30, 10, 0), (31, 11, 2), (32, 11, 1),
                                                 (127, 43, 2)]
    assert m.rows_per_item(254) == 44 and m.rows_per_item(16) == 4 and m.vars_per_item(2) == 0
    for bad in (0, 1, 3, 255, 256, -2):
        with pytest.raises(ValueError):
            m.layout(bad)


@pytest.mark.parametrize("num_bits", m.NUM_BITS)
def test_item_layout(num_bits):
    k, g, pad = m.layout(num_bits)
    wit, first, zero = 7, 100, 0
    v = random.Random(num_bits).randrange(2**num_bits)
    rows, qr, new = m.item(wit, v, num_bits, first, zero)
    assert len(rows) == g + 1 and len(new) == k - 1 and qr == [1] * g + [0]
    flat = [x for r in rows[:g] for x in r] + [rows[g][0]]
    assert flat[:pad + 1] == [zero] * (pad + 1)
    assert flat[pad + 1:3 * g] == list(range(first, first + k - 1))
    assert flat[3 * g] == wit and rows[g][1:] == (zero, zero)
    # accumulator j (from the top) is the witness without its lowest k - 1 - j quads
    assert new == [v >> (2 * (k - 1 - j)) for j in range(k - 1)]


@pytest.mark.parametrize("num_bits", m.NUM_BITS)
def test_rows_hold_iff_in_range(num_bits):
    rnd = random.Random(1000 + num_bits)
    vals = list(m.edge_values(num_bits)) + [rnd.randrange(2**num_bits) for _ in range(8)] + [rnd.randrange(2**num_bits, R) for _ in range(8)]
    for v in vals:
        c = m.Circuit()
        w = c.add_input(v)
        first = c.range_gate(w, num_bits)
        bad = c.first_bad()
        if v < 2**num_bits:
            assert bad == -1, (num_bits, v)
        else:
            assert bad == first, (num_bits, v, bad)  # the first accumulator is >= 4: the item's row 0


def test_a_changed_accumulator_names_its_row():
    c = m.Circuit()
    w = c.add_input(0x123456789abcdef)
    first = c.range_gate(w, 60)
    k, g, pad = m.layout(60)
    nv0 = w + 1
    for j in (0, 1, 2, 3, 14, k - 2):
        d = m.Circuit(values=c.values)
        d.rows, d.q_range = c.rows, c.q_range
        d.values[nv0 + j] = (d.values[nv0 + j] + 5) % R
        p = pad + 1 + j
        # position p sits on row p // 3; as a row's first wire it is also the previous row's a_next
        assert d.first_bad() == first + (p // 3 - 1 if p % 3 == 0 else p // 3)
