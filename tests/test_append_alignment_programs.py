"""CPU: the programs of the alignment sweep (tests/alignment_programs.py) on the oracle alone.  Every program is satisfiable, visits
each of the 64 targets with every batch and shape, keeps at least 64 rows and 64 Variables of its composer's fixed capacity free
behind every call and 16 rows / 4 Variables in front of it (tests/capacity_views.py, room: asserted by the replay itself), and is the
same circuit on another witness seed.  No GPU is needed, but the built library is: the weighted sum's program asks
pg_weighted_sum_geometry for its tile, as tests/test_weighted_sum_cpu.py does."""
import numpy as np
import pytest

from tests import alignment_programs as ap
from tests import capacity_views as cv


# 2 g + 2 rows an interval, 2 n + 4 a decomposition, 4 a select_one, 10 or 8 a fused mix; add_input_batch has no rows at all
EVEN_ROWS_ONLY = {"interval_gate_batch", "interval_gate_ragged_batch", "scalar_decomposition_batch", "conditionally_select_one_batch",
                  "scalar_mix_batch", "scalar_mix_batch_failing", "add_input_batch"}


def test_every_kind_has_a_capacity():
    assert set(ap.CAPACITY) == {k.name for k in ap.KINDS}


def test_every_batched_append_is_swept():
    """a batched append added to StandardComposer must join KINDS"""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "plonk_gadgets_amd", "composer.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "StandardComposer")
    appends = {f.name for f in cls.body if isinstance(f, ast.FunctionDef) and not f.name.startswith("_")
               and (f.name.endswith("_batch") or f.name == "is_less_equal_each")}
    assert appends <= {k.name for k in ap.KINDS}, appends - {k.name for k in ap.KINDS}


@pytest.mark.parametrize("kind", ap.KINDS, ids=repr)
def test_program_on_the_oracle(kind):
    both, plan = ap.replay_on_oracle(kind, 1)
    n, nv = both.ora.n, both.ora.num_vars
    gates, variables = ap.CAPACITY[kind.name]
    assert gates - n >= cv.ROOM_BEHIND and variables - nv >= cv.ROOM_BEHIND, (kind.name, n, nv)
    assert gates - n < 4096 + cv.ROOM_BEHIND and variables - nv < 4096 + cv.ROOM_BEHIND, f"{kind.name} ends at {n} rows, {nv} Variables"
    # all 64 targets, every batch and shape at each, and the tile run at the 16 row residues
    seen = {(n0 % 16, v0 % 4, b, s) for (_, n0, _, v0, _), (_, _, b, s) in zip(both.calls, ap.targets(kind))}
    assert len(both.calls) == 64 * 3 * kind.shapes + 16 and len(plan) == 2 * len(both.calls)
    assert {(r, v, b, s) for r in range(16) for v in range(4) for b in ap.BATCHES for s in range(kind.shapes)} <= seen
    assert {n0 % 16 for _, n0, *_ in both.calls[-16:]} == set(range(16))
    for (what, n0, n1, v0, v1), (r, v, b, s) in zip(both.calls, ap.targets(kind)):
        assert (n0 % 16, v0 % 4) == (r, v), what
        assert n1 > n0 or kind.name == "add_input_batch", what
    # a total of rows that is odd at some batch, unless every item of the kind has an even number of rows
    odd = any((n1 - n0) % 2 for _, n0, n1, *_ in both.calls)
    assert odd != (kind.name in EVEN_ROWS_ONLY), kind
    assert both.first_bad() == -1, (kind.name, both.first_bad())      # (an item that stops at its error leaves only rows that hold)
    other, other_plan = ap.replay_on_oracle(kind, 2)
    assert [p[1:] for p in plan] == [p[1:] for p in other_plan]
    ea, eb = both.ora.export(), other.ora.export()
    for k in ("q_m", "q_l", "q_r", "q_o", "q_c", "w_l", "w_r", "w_o"):
        assert np.array_equal(ea[k], eb[k]), k
    assert both.wid.q_range_rows == other.wid.q_range_rows
    assert kind.name == "constrain_to_constant_batch" or not np.array_equal(ea["var_values"], eb["var_values"])
