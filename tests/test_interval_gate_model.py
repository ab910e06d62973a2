"""CPU: the model of the interval gadget (tests/interval_gate_model.py) against its specification in Python integers: the
layout for every pad and g, "every row of the item holds -- widget rows and both terminal rows -- iff lo <= v <= hi" on the edge
witnesses and bounds, and what each precondition on the bounds is for."""
import random

import pytest

from tests import interval_gate_model as im
from tests import range_gate_model as m

R = im.R


def holds(v, lo, hi, num_bits, checked=True):
    """does every row of the one item hold?  (and: the first failing row is row 0 of a half, the terminal rows always hold)"""
    c = im.Circuit()
    w = c.add_input(v)
    first = c.interval_gate(w, lo, hi, num_bits, checked)
    bad = c.first_bad()
    g = im.layout(num_bits)[1]
    for h in (0, 1):
        t = first + h * (g + 1) + g
        assert im.arith_holds(c.sel[t], *(c.values[x] for x in c.rows[t]))
    assert bad in (-1, first, first + g + 1), bad
    return bad == -1


def test_layout_covers_every_pad_with_one_and_with_several_rows():
    seen = {(im.layout(b)[2], im.layout(b)[1] > 1) for b in im.NUM_BITS}
    assert seen == {(p, many) for p in (0, 1, 2) for many in (False, True)}
    assert [im.layout(b) for b in im.NUM_BITS] == [(1, 1, 2), (2, 1, 1), (3, 1, 0), (4, 2, 2), (31, 11, 2), (32, 11, 1), (126, 42, 0)]
    assert im.rows_per_item(64) == 24 and im.vars_per_item(64) == 64 and im.rows_per_item(2) == 4 and im.vars_per_item(2) == 2
    for bad in (0, 1, 3, 253, 254, 256, -2):
        with pytest.raises(ValueError):
            im.layout(bad)
    for lo, hi, bits in ((6, 5, 8), (0, 256, 8), (0, R, 8), (0, 4, 2)):
        with pytest.raises(ValueError):
            im.check_bounds(lo, hi, bits)
    im.check_bounds(0, 255, 8)
    im.check_bounds(R - 4, R - 1, 2)


@pytest.mark.parametrize("num_bits", im.NUM_BITS)
def test_item_layout(num_bits):
    k, g, pad = im.layout(num_bits)
    wit, first, zero = 7, 100, 0
    rnd = random.Random(num_bits)
    lo = rnd.randrange(2**num_bits)
    hi = lo + rnd.randrange(2**num_bits)
    v = rnd.randrange(lo, hi + 1)
    rows, sel, qr, new = im.item(wit, v, lo, hi, num_bits, first, zero)
    assert len(rows) == 2 * (g + 1) and len(new) == 2 * k and qr == ([1] * g + [0]) * 2
    for h, d in ((0, v - lo), (1, hi - v)):
        base, r0 = first + h * k, h * (g + 1)
        flat = [x for r in rows[r0:r0 + g] for x in r] + [rows[r0 + g][0]]
        assert flat[:pad + 1] == [zero] * (pad + 1)
        assert flat[pad + 1:] == list(range(base, base + k))       # the accumulators, then d: P(3g)
        assert rows[r0 + g] == (base + k - 1, wit, zero)
        assert new[h * k:(h + 1) * k] == [d >> (2 * (k - 1 - j)) for j in range(k)]
        assert sel[r0:r0 + g] == [(0, 0, 0, 0, 0)] * g
    assert sel[g] == (0, 1, R - 1, 0, lo) and sel[2 * g + 1] == (0, 1, 1, 0, (-hi) % R)
    # the halves are range_gate items on d, but for the terminal row
    for h, d in ((0, v - lo), (1, hi - v)):
        w_rows, _, accs = m.item(first + h * k + k - 1, d, num_bits, first + h * k, zero)
        assert rows[h * (g + 1):h * (g + 1) + g] == w_rows[:g] and new[h * k:(h + 1) * k - 1] == accs


@pytest.mark.parametrize("num_bits", im.NUM_BITS)
def test_rows_hold_iff_in_interval(num_bits):
    rnd = random.Random(2000 + num_bits)
    cases = im.edge_cases(num_bits)
    assert any(lo == 0 for lo, _ in cases) and any(lo == hi for lo, hi in cases)
    assert any(hi - lo == 2**num_bits - 1 for lo, hi in cases) and any(hi == R - 1 for _, hi in cases)
    for _ in range(4):
        lo = rnd.randrange(R - 2**num_bits)
        cases.append((lo, lo + rnd.randrange(2**num_bits)))
    for lo, hi in cases:
        ws = im.edge_witnesses(lo, hi) + [rnd.randrange(R) for _ in range(4)] + [rnd.randrange(lo, hi + 1) for _ in range(4)]
        for v in ws:
            assert holds(v, lo, hi, num_bits) == (lo <= v <= hi), (num_bits, lo, hi, v)


def test_an_out_of_range_witness_fails_on_row_zero_of_the_negative_half():
    for num_bits in (2, 8, 64, 252):
        g = im.layout(num_bits)[1]
        lo, hi = 10, 10 + 2**num_bits - 2  # (one short of the widest: hi + 1 then fails half 1 alone)
        for v, half in ((lo - 1, 0), (hi + 1, 1), (R - 1, 0), (0, 0)):
            c = im.Circuit()
            first = c.interval_gate(c.add_input(v), lo, hi, num_bits)
            assert c.first_bad() == first + half * (g + 1), (num_bits, v)


@pytest.mark.parametrize("num_bits", (2, 4, 6))
def test_what_the_width_precondition_is_for(num_bits):
    """hi - lo = 2^num_bits, one more than allowed.  A search over every v that can satisfy half 0 or half 1 (d < 2^num_bits
    leaves 2^num_bits candidates on each side) finds NO v outside [lo, hi] that satisfies every row: at this width the two
    differences still add up to hi - lo below r, so soundness survives.  What breaks is the other direction: v = lo and v = hi
    lie in the interval and are refused (the other difference is 2^num_bits itself) -- the statement would be lo < v < hi.  From
    hi - lo = 2^(num_bits + 1) - 1 on nothing satisfies it at all."""
    w = 2**num_bits
    for lo in (0, 9, R - 1 - w):
        hi = lo + w
        cand = {(lo + d) % R for d in range(w)} | {(hi - d) % R for d in range(w)} | {(lo - 1) % R, (hi + 1) % R, 0, R - 1}
        ok = {v for v in cand if holds(v, lo, hi, num_bits, checked=False)}
        assert ok == set(range(lo + 1, hi)), (lo, sorted(ok))
    lo, hi = 3, 3 + 2 * w - 1
    assert not any(holds(v, lo, hi, num_bits, checked=False) for v in range(0, hi + 3))


@pytest.mark.parametrize("num_bits", (2, 8, 252))
def test_what_the_order_precondition_is_for(num_bits):
    """lo > hi as integers: the interval is empty, but where hi - lo wraps to a small field element the rows are satisfied by
    witnesses on both sides of the modulus -- this is the case the library must refuse for soundness"""
    lo, hi = R - 1, 0
    assert holds(R - 1, lo, hi, num_bits, checked=False) and holds(0, lo, hi, num_bits, checked=False)
    with pytest.raises(ValueError):
        im.check_bounds(lo, hi, num_bits)


def test_bounds_near_the_modulus_at_252_bits():
    w = 2**252 - 1
    for lo, hi in ((R - 1 - w, R - 1), (R - 2, R - 1), (R - 1 - w, R - 2)):
        for v in (lo, hi, lo - 1, (hi + 1) % R, 0, R - 1, lo + w // 2):
            assert holds(v, lo, hi, 252) == (lo <= v <= hi), (lo, hi, v)
    # 2^253 < r: the two differences cannot add up across the modulus
    assert 2 * 2**252 < R < 2 * 2**254
