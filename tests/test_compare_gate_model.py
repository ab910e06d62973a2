"""CPU: the model of the comparison gadget (tests/compare_gate_model.py) against its specification in Python integers: the layout
for every pad with one and with several widget rows, the exhaustive truth table at 2 and 4 bits for both `strict` values, directed
values at 64 and 252 bits, the item whose z does not fit (its row 0 fails), and the documented case outside the precondition."""
import pytest

from tests import compare_gate_model as cm
from tests import interval_gate_model as im
from tests import range_gate_model as m

R = cm.R


def one_item(x, y, num_bits, strict):
    """-> (circuit, first row, value of the result Variable, first failing row or -1)"""
    c = cm.Circuit()
    xv, yv = c.add_input(x), c.add_input(y)
    first, res = c.is_less_equal(xv, yv, num_bits, strict)
    g = cm.layout(num_bits)[1]
    assert im.arith_holds(c.sel[first + g], *(c.values[v] for v in c.rows[first + g]))   # the terminal row always holds
    return c, first, c.values[res], c.first_bad()


def test_layout_covers_every_pad_with_one_and_with_several_rows():
    assert [cm.layout(b) for b in cm.NUM_BITS] == [(2, 1, 1), (3, 1, 0), (4, 2, 2), (32, 11, 1), (33, 11, 0), (127, 43, 2)]
    seen = {(cm.layout(b)[2], cm.layout(b)[1] > 1) for b in cm.NUM_BITS}
    assert {p for p, _ in seen} == {0, 1, 2} and {many for _, many in seen} == {False, True}
    assert cm.rows_per_item(64) == 12 and cm.vars_per_item(64) == 33 and cm.rows_per_item(2) == 2 and cm.vars_per_item(2) == 2
    for bad in (0, 1, 3, 63, 253, 254, 256, -2):
        with pytest.raises(ValueError):
            cm.layout(bad)
    assert 2**253 < R   # 2^(num_bits + 1) < r at the widest: z cannot wrap under the precondition


@pytest.mark.parametrize("strict", (False, True))
@pytest.mark.parametrize("num_bits", cm.NUM_BITS)
def test_item_layout(num_bits, strict):
    k, g, pad = cm.layout(num_bits)
    xv, yv, first, zero = 7, 9, 100, 0
    x, y = (3 * 2**num_bits // 7) | 1, 5 * 2**num_bits // 7
    rows, sel, qr, new, res = cm.item(xv, yv, x, y, num_bits, strict, first, zero)
    s = 1 if strict else 0
    z = 2**num_bits + y - x - s
    assert len(rows) == g + 1 and len(new) == k and qr == [1] * g + [0] and res == first
    flat = [v for r in rows[:g] for v in r] + [rows[g][0]]
    assert flat[:pad + 1] == [zero] * (pad + 1)
    assert flat[pad + 1:] == list(range(first, first + k))          # the accumulators, then z: P(3g)
    assert rows[g] == (first + k - 1, yv, xv)
    assert new == [z >> (2 * (k - 1 - kk)) for kk in range(k)] and new[0] == 1 and new[-1] == z
    assert sel[:g] == [(0, 0, 0, 0, 0)] * g and sel[g] == (0, 1, R - 1, 1, (s - 2**num_bits) % R)
    # the widget rows are those of a range_gate item over num_bits + 2 bits on z
    w_rows, _, accs = m.item(first + k - 1, z, num_bits + 2, first, zero)
    assert rows[:g] == w_rows[:g] and new[:-1] == accs


@pytest.mark.parametrize("strict", (False, True))
@pytest.mark.parametrize("num_bits", (2, 4))
def test_truth_table_is_exhaustive_at_small_widths(num_bits, strict):
    for x in range(2**num_bits):
        for y in range(2**num_bits):
            _, _, res, bad = one_item(x, y, num_bits, strict)
            assert bad == -1, (x, y)
            assert res == int(x < y if strict else x <= y), (x, y)


@pytest.mark.parametrize("strict", (False, True))
@pytest.mark.parametrize("num_bits", (64, 252))
def test_directed_values_at_large_widths(num_bits, strict):
    top = 2**num_bits - 1
    mid = 2**(num_bits - 1) + 12345
    cases = [(mid, mid), (mid, mid + 1), (mid, mid - 1), (0, 0), (top, top), (0, top), (top, 0), (0, 1), (1, 0), (top - 1, top),
             (top, top - 1)]
    for x, y in cases:
        _, _, res, bad = one_item(x, y, num_bits, strict)
        assert bad == -1, (x, y)
        assert res == int(x < y if strict else x <= y), (x, y)


@pytest.mark.parametrize("num_bits", cm.NUM_BITS)
def test_a_z_beyond_the_widget_fails_on_row_zero_of_the_item(num_bits):
    """x = 0, y = 3 * 2^num_bits: c(z) = 2^(num_bits + 2) = 2^K does not fit K bits.  The item still has all its rows; the first
    accumulator is 4, so its row 0 is the first that fails"""
    c, first, res, bad = one_item(0, 3 * 2**num_bits, num_bits, False)
    assert res == 4 and bad == first
    c.range_gate(c.add_input(1), 2)      # rows behind it change nothing
    assert c.first_bad() == first


def test_outside_the_precondition_the_result_has_no_meaning():
    """RECORDED, not wanted: x = r - 1 is not below 2^num_bits.  z = 2^num_bits + 0 - (r - 1) = 2^num_bits + 1 in the field, every
    row holds and the result is 1 although x > y as integers.  The gadget does not bound its inputs"""
    for num_bits in cm.NUM_BITS:
        c, _, res, bad = one_item(R - 1, 0, num_bits, False)
        assert bad == -1 and res == 1 and c.values[-1] == 2**num_bits + 1
    # and with the inputs bounded by range_gate, as the precondition asks, the same witness is refused by ITS widget
    c = cm.Circuit()
    xv, yv = c.add_input(R - 1), c.add_input(0)
    first = c.range_gate(xv, 64)
    c.range_gate(yv, 64)
    c.is_less_equal(xv, yv, 64)
    assert c.first_bad() == first
