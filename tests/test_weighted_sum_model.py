"""CPU: the Python-integer model of weighted_sum_ragged_batch (tests/weighted_sum_model.py) against the loop of composer.add calls it
stands for, replayed on the C oracle's composer (tests/weighted_sum_oracle.py): rows, selectors, Variable numbering, values, check()
and the result formula, for segments of 2, 3, 17 and 300 terms, with and without coefficients and constants, a Variable twice in
one segment, zero_var as a term, the edge coefficients and constants, and sums that are 0 mod r; and what the random programs of
tests/test_gpu_weighted_sum.py reach."""
import numpy as np
import pytest

from tests import weighted_sum_model as wm
from tests import weighted_sum_oracle as wso
from tests import widget_oracle as wo

R = wm.R
CASES = wso.cases()


def ints(col):
    return [wo.int_of(l) for l in np.asarray(col).reshape(-1, 4)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_the_oracle_loop(case):
    both = wso.Both(None)
    x, n0, v0, res = wso.run_case(both, case)
    ora = both.ora
    values = [both.value(v) for v in x]
    rows, sel, new, results = wm.item(x, values, case["seg_off"], case["coeffs"], case["constants"], v0)
    terms, segments = len(x), len(case["seg_off"]) - 1
    assert ora.n == n0 + terms - segments and ora.num_vars == v0 + terms - segments
    got = ora.export(n0, v0)
    for j, k in enumerate(("q_m", "q_l", "q_r", "q_o", "q_c")):
        assert ints(got[k]) == [s[j] for s in sel], k
    for j, k in enumerate(("w_l", "w_r", "w_o")):
        assert [int(w) for w in got[k]] == [r[j] for r in rows], k
    assert ints(got["var_values"]) == new
    assert res == results == [v0 + case["seg_off"][s + 1] - s - 2 for s in range(segments)]
    assert ora.check() == -1
    # the results hold the sums
    c = case["coeffs"] or [1] * terms
    k = case["constants"] or [0] * segments
    for s in range(segments):
        b, e = case["seg_off"][s], case["seg_off"][s + 1]
        assert both.value(res[s]) == (k[s] + sum(c[t] * values[t] for t in range(b, e))) % R
    # every row's statement in the model's own words, and the full sigma is a permutation that the oracle can make
    table = {v: val for v, val in zip(x, values)}
    table.update({v0 + i: val for i, val in enumerate(new)})
    assert all(wm.arith_holds(s, *(table[v] for v in r)) for r, s in zip(rows, sel))


def test_a_bumped_term_value_fails_exactly_the_terms_row():
    """the model's statement with one term's input value moved by one: the first failing row is the row that term owns (its segment's
    first row for the segment's first term)"""
    case = CASES[3]
    both = wso.Both(None)
    vs = both.add_input_batch(list(range(100, 100 + len(case["terms"]))))   # every term a Variable of its own
    x = vs
    v0 = both.ora.num_vars
    values = [both.value(v) for v in x]
    rows, sel, new, _ = wm.item(x, values, case["seg_off"], [c or 1 for c in case["coeffs"]], case["constants"], v0)
    table = {v: val for v, val in zip(x, values)}
    table.update({v0 + i: val for i, val in enumerate(new)})
    starts = set(case["seg_off"][:-1])
    for t in (0, 1, 2, 4, 5, 21, 22, 23, 321, len(x) - 1):
        s = max(i for i, o in enumerate(case["seg_off"][:-1]) if o <= t)
        bumped = dict(table)
        bumped[x[t]] = (table[x[t]] + 1) % R
        bad = [i for i, (r, q) in enumerate(zip(rows, sel)) if not wm.arith_holds(q, *(bumped[v] for v in r))]
        assert bad == [t - s - 1 if t not in starts else t - s], (t, bad)


def test_refused_offsets_name_the_first_offending_segment():
    for seg_off, terms, seg in (([1, 3], 3, 0), ([0, 2, 3, 6], 6, 1), ([0, 4, 2, 6], 6, 1), ([0, 2, 4], 5, 1), ([0, 2, 1 << 40], 4, 1)):
        with pytest.raises(ValueError, match=f"segment {seg}$"):
            wm.check_seg_off(seg_off, terms)
    wm.check_seg_off([0, 2, 4], 4)
    wm.check_seg_off([0], 0)


def test_what_the_random_programs_reach():
    """the eight committed seeds of test_gpu_weighted_sum's random programs, on the oracle alone: among them a sum over results of
    a sum, a sum followed by a range gate on its result, and a planted failure on a sum's result (a sum's own rows hold by
    construction wherever the assignments are computed by the side that states them: the failure sits on the row that uses the
    result), which check() names"""
    from tests import weighted_sum_programs as wprog
    reached, planted = set(), 0
    for seed in wprog.SEEDS:
        both = wprog.run_program(None, seed)
        reached |= both.reached
        planted += both.planted
        assert both.first_bad() == (both.planted_row if both.planted else -1), seed
    assert {"sum_of_sums", "sum_then_range_gate", "failure_on_a_sum_result"} <= reached, reached
    assert 0 < planted < len(wprog.SEEDS)
