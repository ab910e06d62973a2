"""GPU: sigma and the f-rows of circuits with is_less_equal rows, against the C oracle's composer with the gadget replayed on it
(tests/compare_gate_oracle.py; tests/test_compare_gate_oracle.py pins that replay against the model).  Compare rows leave no
footprint: their positions -- x and y on the terminal rows among them -- go through the gap kernel and the sort.  Every test builds
its program on both composers (tests/compare_programs.py) and asserts tests/widget_programs.py's assert_device_equals_oracle:
columns, check(), q_range with a sentinel row behind it, wire values, sigma limb for limb at the padded size and at n."""
import random

import pytest

import plonk_gadgets_amd as pg
from tests import compare_gate_model as cm
from tests.compare_programs import CompareBoth
from tests.widget_programs import assert_device_equals_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def composers(engine):
    dev = pg.StandardComposer(engine, 1 << 14, 1 << 15)
    dev.auto_grow()
    return CompareBoth(dev)


def below(num_bits, n, rnd):
    vals = [2**num_bits - 1, 0] + [rnd.randrange(2**num_bits) for _ in range(n)]
    return vals[:n]


@pytest.mark.parametrize("batch", (1, 3, 257))
@pytest.mark.parametrize("num_bits", cm.NUM_BITS)
def test_every_width_behind_an_add_input_batch(engine, num_bits, batch):
    """x > y, x = y (two Variables, and one Variable on both sides) and x < y; strict on the odd widths' turn"""
    rnd = random.Random(num_bits * 1000 + batch)
    both = composers(engine)
    ws = both.add_input_batch(below(num_bits, 2 * batch, rnd))
    xs, ys = ws[:batch], ws[batch:]
    if batch >= 3:
        ys[1] = xs[1]
        xs[2] = both.zero_var
    res = both.is_less_equal_each(xs, ys, num_bits, strict=(num_bits // 2 + batch) % 2 == 1)
    assert all(both.value(r) in (0, 1) for r in res)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)


def test_compare_rows_between_two_footprints(engine):
    """compare rows between two range_check_batch calls with the same bounds, whose footprints would join if nothing lay between them,
    fed with the first one's results; the bits then select in a conditionally_select_zero_batch, and compare rows are the last rows"""
    rnd = random.Random(5)
    both = composers(engine)
    amounts = both.add_input_batch(below(16, 6, rnd))
    rc = both.range_check_batch(50_000, 250_000, [rnd.randrange(300_000) for _ in range(5)])
    bits = both.is_less_equal_each(rc + amounts[:3], rc[1:] + rc[:1] + amounts[3:], 16)
    rc2 = both.range_check_batch(50_000, 250_000, [rnd.randrange(300_000) for _ in range(5)])
    sel = both.conditionally_select_zero_batch(amounts + rc2[:2], bits)
    both.is_less_equal_each(sel[:4], bits[:4], 16, strict=True)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)


@pytest.mark.parametrize("num_bits", (16, 14))
def test_range_segments_merge_when_g_matches_and_split_when_not(engine, num_bits):
    """a range_gate_batch directly in front and an interval_gate_batch directly behind.  At num_bits = 16 the comparison's widget has
    18 bits (k = 9, g = 3) and so have the neighbours: the three calls are one run of q_range items of four rows.  At num_bits = 14
    (16 bits, k = 8, still g = 3) the neighbours take 12 bits (k = 6, g = 2): three segments"""
    rnd = random.Random(num_bits)
    around = 18 if num_bits == 16 else 12
    both = composers(engine)
    ws = both.add_input_batch(below(12, 12, rnd))
    both.range_gate_batch(ws[:5], around)
    n0 = both.ora.n
    bits = both.is_less_equal_each(ws[:6], ws[6:], num_bits)
    assert both.ora.n - n0 == 6 * 4
    both.interval_gate_batch(ws[3:] + bits[:2], 0, 2**around - 1, around)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)
    # an item out of range in the middle call: check() names its row 0, q_range is what it was
    both2 = composers(engine)
    ws = both2.add_input_batch(below(12, 11, rnd) + [3 * 2**num_bits + 1])
    both2.range_gate_batch(ws[:5], around)
    n0 = both2.ora.n
    both2.is_less_equal_each(ws[:5] + [both2.zero_var], ws[6:], num_bits)      # item 5: z = 2^(num_bits + 2) + 1
    both2.interval_gate_batch(ws[3:9], 0, 2**around - 1, around)
    assert both2.first_bad() == n0 + 5 * 4
    assert_device_equals_oracle(both2)
