"""CPU: the random programs with widget rows (tests/widget_programs.py, run_widget_program) on the oracle alone: what the committed
seeds of test_fuzz_widget_programs reach, that a program's public structure does not depend on its witnesses, and that its
witnesses are in range unless a failure is planted."""
import numpy as np
import pytest

from tests import range_gate_model as m
from tests import widget_programs as wp


@pytest.fixture(scope="module")
def programs():
    return {seed: wp.run_widget_program(None, None, seed) for seed in wp.WIDGET_SEEDS}


def test_the_committed_seeds_reach_the_cases(programs):
    calls = dict.fromkeys(wp.WIDGET_CALLS, 0)
    same_g = other_g = 0
    longest_gap = gadget_witnesses = 0
    satisfied, range_then_arithmetic, arithmetic_then_range = [], [], []
    for seed, both in programs.items():
        run = 0
        for prev, (name, items, num_bits, n0, rows) in zip([(None,) * 5] + both.log, both.log):
            if name in wp.WIDGET_CALLS:
                calls[name] += 1
                run += rows
                if prev[0] in wp.WIDGET_CALLS:   # directly behind another widget call: one RangeSeg if g is alike
                    alike = m.layout(prev[2])[1] == m.layout(num_bits)[1]
                    same_g, other_g = same_g + alike, other_g + (not alike)
            elif rows:
                run = 0
            longest_gap = max(longest_gap, run)
        gadget_witnesses += both.gadget_witnesses
        arith, widget = both.ora.check(), both.wid.first_q_range_bad(both.ora)
        assert both.first_bad() == min([x for x in (arith, widget) if x >= 0], default=-1)
        if arith == widget == -1:
            satisfied.append(seed)
        elif 0 <= widget < arith:
            range_then_arithmetic.append(seed)
        elif 0 <= arith < widget:
            arithmetic_then_range.append(seed)
    assert all(c >= 3 for c in calls.values()), calls
    assert same_g >= 1 and other_g >= 1
    assert longest_gap > 4096                    # more than one workgroup of the f-rows' gap kernel
    assert gadget_witnesses >= 100
    assert len(satisfied) >= 3 and len(range_then_arithmetic) >= 3 and len(arithmetic_then_range) >= 1
    big = [s for s in wp.WIDGET_SEEDS if s > 100]
    assert len(big) == 2 and all(max(items for name, items, *_ in programs[s].log if name in wp.WIDGET_CALLS) >= 400 for s in big)


@pytest.mark.parametrize("seed", wp.WIDGET_SEEDS[:6])
def test_other_witnesses_same_circuit(programs, seed):
    """another wit_seed: the same rows on the same Variables with the same selectors and the same q_range (what a witness refresh
    relies on), other assignments, and the same verdict -- -1 where nothing is planted, the planted row otherwise"""
    a, b = programs[seed], wp.run_widget_program(None, None, seed, wit_seed=5000 + seed)
    ea, eb = a.ora.export(), b.ora.export()
    for k in ("q_m", "q_l", "q_r", "q_o", "q_c", "w_l", "w_r", "w_o"):
        assert np.array_equal(ea[k], eb[k]), k
    assert a.wid.q_range_rows == b.wid.q_range_rows and [c[:2] for c in a.log] == [c[:2] for c in b.log]
    assert not np.array_equal(ea["var_values"], eb["var_values"])
    assert a.first_bad() == b.first_bad()
