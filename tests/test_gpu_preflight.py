"""GPU: the preflight of the appends on device arrays -- one pass per array, one copy back, one host synchronisation -- seen through what
it decides: which rebuilds after clear_witness are found in place (the digest of the arrays), and which calls are refused (the
largest Variable, the call's own preconditions).

  * what the digest tells apart, three items behind eight inputs: two entries of one array exchanged, the two arrays of a call
    exchanged, two items' bounds exchanged, two coefficients exchanged -- each rebuild finds nothing in place and ends the refresh, and
    the same arrays twice in a row are in place again;
  * the end of the kernels (a wave's sum, lane 0's atomics) and their stride: 1, 64, 65 and 257 entries (one lane, one wave, two waves,
    two workgroups) and one entry more than the whole grid's lanes, so that a lane takes a second one; the offender is the LAST entry;
  * one append of more entries than the grid has lanes, in place on an equal rebuild and not with its first and last entries exchanged."""
import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth

pytestmark = pytest.mark.gpu

S = pg.BlsScalar.from_int
R = synth.Q
N_INPUTS = 8


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def tv(xs):
    return torch.tensor(xs, dtype=torch.int64, device="cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def scalars(ints):
    return t(synth.scalars_from_ints(ints))


def inputs(dev, seed):
    """eight allocated inputs in 1 .. 60000 -> the first one's Variable"""
    return dev.add_input_batch(scalars([1 + int(v) % 60_000 for v in synth.splitmix64(N_INPUTS, seed)]))


def entries(n, workgroups_per_cu):
    """"stride": one entry more than a grid of that many workgroups per CU has lanes"""
    return 256 * workgroups_per_cu * torch.cuda.get_device_properties(0).multi_processor_count + 1 if n == "stride" else n


# ---- what the digest tells apart ------------------------------------------------------------------------------------------------------
def maybe_equal(dev, first, changed):
    a = [first + 1, first, first + 2] if changed else [first, first + 1, first + 2]
    dev.maybe_equal_batch(tv(a), tv([first + 3, first + 4, first + 5]))


def select_zero(dev, first, changed):
    a, b = tv([first, first + 1, first + 2]), tv([first + 3, first + 4, first])
    dev.conditionally_select_zero_batch(*((b, a) if changed else (a, b)))


def interval_ragged(dev, first, changed):
    lo, hi = ([1, 0, 1], [2**16, 2**16 - 1, 60_001]) if changed else ([0, 1, 1], [2**16 - 1, 2**16, 60_001])
    dev.interval_gate_ragged_batch(tv([first + 2, first + 3, first + 4]), scalars(lo), scalars(hi), 16)


def weighted_sum(dev, first, changed):
    co = [5, R - 1, 1, 0, 3, 2] if changed else [3, R - 1, 1, 0, 5, 2]
    dev.weighted_sum_ragged_batch(tv([first, first + 1, first + 2, first + 3, first + 4, first + 1]), tv([0, 2, 4, 6]), scalars(co),
                                  scalars([9, 0, R - 1]))


@pytest.mark.parametrize("call", [maybe_equal, select_zero, interval_ragged, weighted_sum], ids=lambda c: c.__name__)
def test_the_digest_tells_exchanged_entries_apart(engine, call):
    dev = pg.StandardComposer(engine, 1 << 10, 1 << 10)
    call(dev, inputs(dev, 1), False)
    rows = dev.circuit_size() - 3
    assert rows > 0
    # the changed arrays against the original, the original against the changed: another circuit each time
    for build, changed in enumerate((True, False)):
        dev.clear_witness()
        call(dev, inputs(dev, 2 + build), changed)
        assert dev.refresh_stats() == (0, rows, False), (build, dev.refresh_stats())
    dev.clear_witness()
    call(dev, inputs(dev, 4), False)
    assert dev.refresh_stats() == (rows, 0, True)
    dev.close()


# ---- the kernels' last lanes: the offender is the last entry ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(engine):
    """a composer of eight inputs that every refused call leaves as it was -> (composer, first input)"""
    dev = pg.StandardComposer(engine, 1 << 10, 1 << 10)
    first = inputs(dev, 7)
    yield dev, first
    dev.close()


def refused(dev, match, call, *args):
    state = dev.circuit_size(), dev.num_variables()
    with pytest.raises(pg.PgError, match=match) as e:
        call(*args)
    assert e.value.status == 2
    assert (dev.circuit_size(), dev.num_variables()) == state


EDGES = [1, 64, 65, 257, "stride"]


@pytest.mark.parametrize("n", EDGES)
def test_an_unknown_variable_in_the_last_entry(small, n):
    dev, first = small
    n = entries(n, 8)  # (max_variable_kernel: eight workgroups per CU)
    a = torch.full((n,), first, dtype=torch.int64, device="cuda:0")
    a[-1] = dev.num_variables()
    refused(dev, f"unknown Variable {dev.num_variables()} ", dev.boolean_gate_batch, a)


@pytest.mark.parametrize("n", EDGES)
def test_min_above_max_in_the_last_item(small, n):
    dev, first = small
    n = entries(n, 2)  # (interval_bounds_kernel: two workgroups per CU)
    lo, hi = scalars([0, 3])
    lo_v, hi_v = lo.repeat(n, 1), hi.repeat(n, 1)
    lo_v[-1], hi_v[-1] = hi, lo
    refused(dev, f"of 1 items .* the first is item {n - 1}\\)", dev.interval_gate_ragged_batch,
            torch.full((n,), first, dtype=torch.int64, device="cuda:0"), lo_v, hi_v, 8)


@pytest.mark.parametrize("n", EDGES)
def test_the_modulus_as_the_last_constant(small, n):
    dev, first = small
    n = entries(n, 2)  # segments of two terms (weighted_sum_check_kernel: two workgroups per CU)
    ks = torch.zeros((n, 4), dtype=torch.int64, device="cuda:0")
    ks[-1] = t(np.array([R >> (64 * j) & (2**64 - 1) for j in range(4)], dtype=np.uint64))
    refused(dev, f"constant {n - 1} is not reduced", dev.weighted_sum_ragged_batch,
            torch.full((2 * n,), first, dtype=torch.int64, device="cuda:0"), torch.arange(0, 2 * n + 1, 2, dtype=torch.int64, device="cuda:0"),
            None, ks)


# ---- one append of more entries than the grid has lanes -------------------------------------------------------------------------------
def test_an_append_over_the_stride_is_found_in_place(engine):
    n = entries("stride", 8)
    dev = pg.StandardComposer(engine, n + 64, 64)

    def build(seed, exchanged):
        first = inputs(dev, seed)
        a = torch.full((n,), first, dtype=torch.int64, device="cuda:0")
        a[0], a[-1] = (first + 2, first + 1) if exchanged else (first + 1, first + 2)
        dev.boolean_gate_batch(a)

    build(1, False)
    assert dev.circuit_size() == 3 + n
    dev.clear_witness()
    build(2, False)
    assert dev.refresh_stats() == (n, 0, True)
    dev.clear_witness()
    build(3, True)
    assert dev.refresh_stats() == (0, n, False)
    dev.close()
