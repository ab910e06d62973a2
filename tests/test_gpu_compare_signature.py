"""GPU: what the signature of is_less_equal_each protects in a witness refresh (pg_composer_clear_witness).  The method's name does
not end in _batch, so tests/test_gpu_clear_witness.py's table of batched appends does not hold it; this file asks the same of it.
The SAME call on other witnesses finds all its rows in place, writes none again, and leaves the composer the oracle's would be, its
first failing row too (the gadget replayed on the oracle by tests/compare_gate_oracle.py).  A DIFFERENT call at the same place with
the same batch -- `strict` flipped, another num_bits, x and y swapped, range_gate_batch at num_bits + 2 on as many Variables, which
writes rows of the very same shape -- finds nothing in place and ends the refresh."""
import random

import numpy as np
import pytest

import plonk_gadgets_amd as pg
from tests.compare_programs import CompareBoth

pytestmark = pytest.mark.gpu

COLS = ("q_m", "q_l", "q_r", "q_o", "q_c", "w_l", "w_r", "w_o", "var_values")
NUM_BITS, BATCH, DUMMY_ROWS = 16, 5, 3
ROWS = BATCH * 4     # k = 9 quads, g = 3 widget rows and the terminal row


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def same(dev, ora):
    """all nine columns, every limb"""
    got, exp = dev.export(), ora.export()
    assert dev.circuit_size() == ora.n and dev.num_variables() == ora.num_vars
    for k in COLS:
        assert got[k].shape == exp[k].shape, k
        if not np.array_equal(got[k], exp[k]):
            raise AssertionError(f"{k} differs first at {np.argwhere(got[k] != exp[k])[0].tolist()}")


def build(both, seed, call, planted=False):
    """ten inputs below 2^16 (x of item 3 equal to its y; planted: item 2 is 0 against 3 * 2^16 + 1), then the append"""
    rnd = random.Random(seed)
    vals = [rnd.randrange(2**NUM_BITS) for _ in range(2 * BATCH)]
    vals[3] = vals[BATCH + 3]
    if planted:
        vals[2], vals[BATCH + 2] = 0, 3 * 2**NUM_BITS + 1
    ws = both.add_input_batch(vals)
    call(both, ws[:BATCH], ws[BATCH:])


def the_call(both, xs, ys):
    both.is_less_equal_each(xs, ys, NUM_BITS, False)


OTHERS = {
    "strict_flipped": lambda both, xs, ys: both.is_less_equal_each(xs, ys, NUM_BITS, True),
    "num_bits_changed": lambda both, xs, ys: both.is_less_equal_each(xs, ys, NUM_BITS + 2, False),
    "x_and_y_swapped": lambda both, xs, ys: both.is_less_equal_each(ys, xs, NUM_BITS, False),
    "range_gate_batch": lambda both, xs, ys: both.range_gate_batch(xs, NUM_BITS + 2),
}


def test_the_same_call_on_other_witnesses_is_found_in_place(engine):
    dev = pg.StandardComposer(engine, 1 << 11, 1 << 12)
    build(CompareBoth(dev), 1, the_call)
    assert dev.circuit_size() == DUMMY_ROWS + ROWS and dev.check() == -1
    for seed, planted in ((2, False), (3, True), (4, False)):
        dev.clear_witness()
        both = CompareBoth(dev)
        build(both, seed, the_call, planted)
        assert dev.refresh_stats() == (ROWS, 0, True)
        same(dev, both.ora)
        assert dev.check() == both.first_bad() == (DUMMY_ROWS + 2 * 4 if planted else -1)
        assert np.array_equal(dev.materialize()["q_range"].cpu().numpy().view(np.uint64), both.wid.q_range_column(both.ora))
        assert dev.copy_constraints_hold()
    dev.close()


@pytest.mark.parametrize("other", sorted(OTHERS))
def test_a_different_call_at_the_same_place_ends_the_refresh(engine, other):
    for first, second in ((the_call, OTHERS[other]), (OTHERS[other], the_call)):
        dev = pg.StandardComposer(engine, 1 << 11, 1 << 12)
        build(CompareBoth(dev), 10, first)
        dev.clear_witness()
        both = CompareBoth(dev)
        build(both, 11, second)
        kept, rewritten, refreshing = dev.refresh_stats()
        assert kept == 0 and rewritten == dev.circuit_size() - DUMMY_ROWS and not refreshing, (other, kept, rewritten, refreshing)
        same(dev, both.ora)
        assert dev.check() == both.first_bad() == -1
        assert np.array_equal(dev.materialize()["q_range"].cpu().numpy().view(np.uint64), both.wid.q_range_column(both.ora))
        dev.clear_witness()   # ... and what the second left is its own: the same call again is a refresh
        build(CompareBoth(dev), 12, second)
        assert dev.refresh_stats() == (dev.circuit_size() - DUMMY_ROWS, 0, True)
        dev.close()
