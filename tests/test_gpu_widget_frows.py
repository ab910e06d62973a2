"""GPU: sigma and the f-rows of circuits with range_gate / interval_gate rows, against the C oracle's composer with the widgets
replayed on it (tests/widget_oracle.py; tests/test_widget_oracle.py pins that replay against the two models).  Widget rows leave no
footprint: their positions go through the gap kernel, the sparse list, the link and the splice kernels of csrc/permutation.hpp, and
copy_constraints_hold() cannot tell a sigma that links too little.  Every test builds its program on both composers
(tests/widget_programs.py, Both) and asserts assert_device_equals_oracle: columns, check(), q_range with a sentinel row behind it,
wire values, sigma limb for limb at the padded size and at n, again with the sparse list reserved too small, and sigma's
size-independent properties.  The shapes are the smallest that reach each structure."""
import random

import pytest

import plonk_gadgets_amd as pg
from tests import interval_gate_model as im
from tests import range_gate_model as m
from tests.widget_programs import Both, assert_device_equals_oracle

pytestmark = pytest.mark.gpu

R = m.R


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def composers(engine):
    dev = pg.StandardComposer(engine, 1 << 14, 1 << 15)
    dev.auto_grow()
    return Both(dev)


def witnesses(both, values):
    """Variables holding `values`, from two earlier calls: the even ones of an add_input_batch, the odd ones the results of a
    mul_batch (inputs times a Variable that holds 1) -- rows in front of the widgets, witnesses that sit on other rows' wires"""
    ev, od = list(values[0::2]), list(values[1::2])
    out = [0] * len(values)
    out[0::2] = both.add_input_batch(ev)
    if od:
        one = both.add_input_batch([1])[0]
        out[1::2] = both.mul_batch(1, both.add_input_batch(od), [one] * len(od), 0)
    return out


def in_range(num_bits, n, rnd):
    vals = [2**num_bits - 1, 0] + [rnd.randrange(2**num_bits) for _ in range(n)]
    return vals[:n]


def interval_bounds(num_bits, n, per_item, rnd):
    if not per_item:
        lo = rnd.randrange(1, R - 2**num_bits)
        return [(lo, lo + rnd.randrange(2**num_bits))] * n
    out = im.edge_cases(num_bits)
    rnd.shuffle(out)
    while len(out) < n:
        lo = rnd.randrange(R - 2**num_bits)
        out.append((lo, lo + rnd.randrange(2**num_bits)))
    return out[:n]


def inside(bounds, rnd):
    return [(lo, hi, rnd.randrange(lo, hi + 1))[i % 3] for i, (lo, hi) in enumerate(bounds)]


def interval_call(both, ws, bounds, num_bits, per_item):
    if per_item:
        both.interval_gate_ragged_batch(ws, [b[0] for b in bounds], [b[1] for b in bounds], num_bits)
    else:
        both.interval_gate_batch(ws, bounds[0][0], bounds[0][1], num_bits)


# ---- every width x batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (1, 3, 257))
@pytest.mark.parametrize("num_bits", m.NUM_BITS)
def test_range_gate_batch_every_width(engine, num_bits, batch):
    rnd = random.Random(num_bits * 1000 + batch)
    both = composers(engine)
    both.range_gate_batch(witnesses(both, in_range(num_bits, batch, rnd)), num_bits)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)


@pytest.mark.parametrize("per_item", (False, True), ids=("one_pair", "pair_per_item"))
@pytest.mark.parametrize("batch", (1, 3, 257))
@pytest.mark.parametrize("num_bits", im.NUM_BITS)
def test_interval_gate_batch_every_width(engine, num_bits, batch, per_item):
    rnd = random.Random(num_bits * 1000 + batch * 2 + per_item)
    both = composers(engine)
    bounds = interval_bounds(num_bits, batch, per_item, rnd)
    interval_call(both, witnesses(both, inside(bounds, rnd)), bounds, num_bits, per_item)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)


# ---- one gap across two workgroups of the gap kernel (4096 rows each) -------------------------------------------------------------
def test_one_call_is_a_gap_of_two_workgroups(engine):
    """400 items of 64 bits: 4800 widget rows in one range_gate_batch, ending in the middle of the second workgroup's rows"""
    rnd = random.Random(64)
    both = composers(engine)
    ws = witnesses(both, in_range(64, 400, rnd))
    n0 = both.ora.n
    both.range_gate_batch(ws, 64)
    assert both.ora.n - n0 == 4800 and both.first_bad() == -1
    assert_device_equals_oracle(both)


def test_two_adjacent_calls_are_one_gap(engine):
    """the same 4800 rows from a range_gate_batch of 200 and an interval_gate_batch of 100 right behind it: one gap, and g alike"""
    rnd = random.Random(65)
    both = composers(engine)
    ws = witnesses(both, in_range(64, 300, rnd))
    n0 = both.ora.n
    both.range_gate_batch(ws[:200], 64)
    both.interval_gate_batch(ws[200:], 0, 2**64 - 1, 64)
    assert both.ora.n - n0 == 4800 and both.first_bad() == -1
    assert_device_equals_oracle(both)


# ---- hot Variables --------------------------------------------------------------------------------------------------------------
def test_one_variable_is_the_witness_of_every_item(engine):
    """257 and 514 terminal positions in one cycle, behind the position on the row that made the Variable"""
    both = composers(engine)
    w = witnesses(both, [5, 40_000])[1]
    both.range_gate_batch([w] * 257, 16)
    both.interval_gate_batch([w] * 257, 39_000, 41_000, 16)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)


def test_zero_var_is_a_witness(engine):
    """zero_var (value 0, in range): a range item's terminal row is then zero_var on all four wires"""
    both = composers(engine)
    zero = both.zero_var
    w = witnesses(both, [7, 9])
    both.range_gate(zero, 8)
    both.range_gate_batch([zero, w[0], zero, zero, w[1]], 6)
    both.interval_gate_batch([zero, zero, w[1]], 0, 15, 4)
    both.interval_gate_ragged_batch([w[0], zero], [3, 0], [10, 0], 4)
    both.interval_gate(zero, 0, 3, 2)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)


# ---- between footprints ---------------------------------------------------------------------------------------------------------
def n_range_check(both, items, rnd):
    """range_check_batch, twice with the same bounds: 83 rows an item, one footprint if nothing lay between"""
    return both.range_check_batch(50_000, 250_000, [rnd.randrange(300_000) for _ in range(items)])


def n_select_zero(both, items, rnd):
    """conditionally_select_zero_batch: a row an item, the template route"""
    pool = both.add_input_batch([rnd.randrange(2) for _ in range(16)])
    return both.conditionally_select_zero_batch([rnd.choice(pool) for _ in range(items)], [rnd.choice(pool) for _ in range(items)])


def n_max_bound_ragged(both, items, rnd):
    """max_bound_ragged_batch: 2 n + 5 rows an item with n from 21 to 41, the ragged ladder"""
    bounds = [rnd.randrange(1 << 20, 1 << 40) for _ in range(items)]
    return both.max_bound_ragged_batch(bounds, [rnd.randrange(2 * b) for b in bounds])


def n_scalar_mix(both, items, rnd, failing=()):
    """scalar_mix_batch: 10 rows an item; an item in `failing` has v = 0 and stops at is_non_zero's error"""
    v = [0 if i in failing else rnd.randrange(1, R) for i in range(items)]
    y, s, a, b = ([rnd.choice([0, 1, rnd.randrange(R)]) for _ in range(items)] for _ in range(4))
    res, nerr = both.scalar_mix_batch(v, y, s, a, b)
    assert nerr == len(failing)
    return [r[1] for r in res]


# (neighbour, items for a closed-form segment: at least 4096 rows)
NEIGHBOURS = {"range_check": (n_range_check, 50), "select_zero": (n_select_zero, 4100), "max_bound_ragged": (n_max_bound_ragged, 90),
              "scalar_mix": (n_scalar_mix, 420)}


@pytest.mark.parametrize("long", (False, True), ids=("5_items", "closed_form"))
@pytest.mark.parametrize("neighbour", sorted(NEIGHBOURS))
def test_widget_rows_between_two_footprints(engine, neighbour, long):
    """widget rows as the first rows behind the dummy rows, between two calls of one gadget whose footprints would join if nothing
    lay between them, and as the last rows of the circuit; the widgets' witnesses are inputs and the 0 / 1 results of the call
    in front"""
    rnd = random.Random(len(neighbour) * 2 + long)
    call, items = NEIGHBOURS[neighbour]
    items = items if long else 5
    both = composers(engine)
    ws = both.add_input_batch(in_range(16, 7, rnd))
    assert both.ora.n == 3
    both.range_gate_batch(ws, 16)
    n0 = both.ora.n
    first = call(both, items, rnd)
    assert not long or both.ora.n - n0 >= 4096
    both.range_gate_batch(ws[:3] + first[:4], 16)
    if neighbour == "scalar_mix":
        second = call(both, items, rnd, failing=(items // 2,))
    else:
        second = call(both, items, rnd)
    both.interval_gate_batch(second[-3:] + ws[3:], 0, 2**16 - 1, 16)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)


# ---- foreign witnesses ----------------------------------------------------------------------------------------------------------
def test_witnesses_from_earlier_batched_gadgets(engine):
    """the widgets' witnesses are positions of closed-form segments: results of range_check_batch, maybe_equal_batch and add_batch,
    and bit Variables from inside ladder items (Variables the items made themselves, spliced with gap rows)"""
    rnd = random.Random(8)
    both = composers(engine)
    inputs = both.add_input_batch([rnd.randrange(256) for _ in range(12)])
    nv0 = both.ora.num_vars
    rc = both.range_check_batch(50_000, 250_000, [rnd.randrange(300_000) for _ in range(60)])   # 4980 rows
    nv1 = both.ora.num_vars
    meq = both.maybe_equal_batch(inputs[:6] + inputs[:2], inputs[6:] + inputs[:2])
    sums = both.add_batch(1, inputs[:6], 1, inputs[6:], 3)                                        # below 2^9 + 3
    per_item = (nv1 - nv0) // 60
    bits = []
    for item in (0, 31, 59):    # Variables inside these items that hold 0 or 1, the result aside
        inner = [v for v in range(nv0 + item * per_item + 1, nv0 + (item + 1) * per_item) if v not in rc and both.value(v) <= 1]
        bits += [inner[0], inner[len(inner) // 2], inner[-1]]
    both.range_gate_batch(rc[:20] + bits + meq + sums, 16)
    both.interval_gate_batch(sums + rc[20:] + bits[::-1] + meq, 0, 2**10, 12)
    both.range_gate(rc[0], 2)
    both.interval_gate(bits[0], 0, 1, 2)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)


# ---- segment merging ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planted", ("nowhere", "last_call", "first_call"))
def test_range_segments_merge_across_calls(engine, planted):
    """range_gate_batch(16), interval_gate_batch(16) and a single range_gate(16) right behind one another (g alike), then
    range_gate_batch(8) (another g), a constrain_to_constant, and range_gate_batch(8) again; an out-of-range witness planted in the
    last call and, separately, in the first: q_range is what it was, check() names the item's first row"""
    rnd = random.Random(16)
    both = composers(engine)
    wide = both.add_input_batch(in_range(16, 9, rnd) + ([2**16] if planted == "first_call" else [77]))
    narrow = both.add_input_batch(in_range(8, 9, rnd) + ([R - 1] if planted == "last_call" else [77]))
    rows = []
    for call in (lambda: both.range_gate_batch(wide[5:], 16), lambda: both.interval_gate_batch(wide[:5], 0, 2**16 - 1, 16),
                 lambda: both.range_gate(wide[0], 16), lambda: both.range_gate_batch(narrow[:4], 8),
                 lambda: both.constrain_to_constant(both.zero_var, 0), lambda: both.range_gate_batch(narrow[4:], 8)):
        rows.append(both.ora.n)
        call()
    expected = {"nowhere": -1, "first_call": rows[0] + 4 * m.rows_per_item(16), "last_call": rows[5] + 5 * m.rows_per_item(8)}
    assert both.first_bad() == expected[planted]
    assert_device_equals_oracle(both)
