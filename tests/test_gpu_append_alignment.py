"""GPU: every composer append at every line alignment, with canaries ("Alignments").

An append's writers derive their store pattern from the address of the call's first row and first Variable: emit_kernel skips `mis`
lanes so that its selector sweep starts on a 128-byte line, pairs wire rows from a 16-byte boundary (`shift`, `pmis`; the odd head
and tail row of a call are single 8-byte stores) and counts Variables from the line before the tile's first one (`smis`);
weighted_sum_write_kernel has a head / tail pairing of its own; a tile after the first takes its pattern from its own first row.  One
test per kind of append visits all 64 targets -- (first row) mod 16 x (first Variable) mod 4 -- with batches 1, 2 and 3 of each
shape, then a batch of the tile width + 1 at the 16 row residues (tests/alignment_programs.py), on ONE composer of fixed capacity
beside one oracle replay.  Around every call tests/capacity_views.py arms the whole capacity: what was live before the call must be
bit for bit unchanged after it, what lies behind the composer's new end must still hold the canary.  So a store one row before a
call, one pair behind it, or a variable line written past the end fails at the call that made it, named by kind, alignment and batch.

No composer here has auto_grow on, and before each call the room is asserted (capacity_views.room): at least 64 rows and Variables of
spare capacity behind the call's end, 16 rows and 4 Variables in front of its start -- a stray store of a whole skipped-lane sweep
stays inside the allocation on either side and shows as a mismatch.

After the sweep of a kind: the whole circuit against the oracle (columns from row 0, check(), q_range, wire values, sigma at the
padded size and through the short sparse list); the values-only refresh (clear_witness, the same program on other witnesses, armed
as before: the eight row columns bit for bit as they were, the variable table the second oracle's); and the f-rows
(pg_composer_materialize, pg_composer_permutation at padded_n and at n) into canary-guarded outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import _lib
from tests import alignment_programs as ap
from tests import capacity_views as cv
from tests import widget_programs as wp

pytestmark = pytest.mark.gpu

WITNESSES, OTHER_WITNESSES = 1, 2
ROW_COLS = cv.ROW_COLS
GUARD_ROWS = cv.ROOM_BEHIND


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def assert_whole_circuit(both):
    """export() from row 0 against the oracle's; a mismatch is named as call / target alignment / batch"""
    got, exp = both.dev.export(), both.ora.export()
    for k in ROW_COLS + ("var_values",):
        assert got[k].shape == exp[k].shape, k
        if not np.array_equal(got[k], exp[k]):
            differs = got[k] != exp[k]
            at = int(np.argwhere(differs.any(axis=1) if differs.ndim == 2 else differs)[0])
            raise AssertionError(f"{k} differs from the oracle's first at {at}: {ap.describe(both, k, at)}")
    wp.assert_device_equals_oracle(both)


def assert_f_rows_guarded(both):
    """materialize once, every output GUARD_ROWS longer than the circuit and canary-filled; permutation at padded_n and at n into
    canary-guarded buffers: nothing past the last row written, the values the oracle's (var_values[w] for the wire-value columns)"""
    dev, ora = both.dev, both.ora
    n = dev.circuit_size()
    names = ("q_4", "q_arith", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add")
    vals = ("w_l_value", "w_r_value", "w_o_value", "w_4_value")
    t = {k: torch.full((n + GUARD_ROWS, 4), cv.CANARY, dtype=torch.int64, device="cuda:0") for k in names + vals}
    t["w_4"] = torch.full((n + GUARD_ROWS,), cv.CANARY, dtype=torch.int64, device="cuda:0")
    assert dev._lib.pg_composer_materialize(dev._h, C.byref(_lib.FullColumnsC(**{k: v.data_ptr() for k, v in t.items()}))) == 0
    dev.sync()
    torch.cuda.synchronize()
    for k, v in t.items():
        assert bool((v[n:] == cv.CANARY).all()), f"{k}: rows past the circuit's last were written"
    full = ora.full_columns()
    exp = {"q_4": full["q_4"], "q_arith": full["q_arith"], "q_range": both.wid.q_range_column(ora), "w_4": full["w_4"]}
    for k in names:
        got = t[k][:n].cpu().numpy().view(np.uint64)
        e = exp.get(k, np.zeros((n, 4), dtype=np.uint64))
        if not np.array_equal(got, e):
            at = int(np.argwhere((got != e).any(axis=1))[0])
            raise AssertionError(f"{k} differs from the oracle's first at row {at}: {ap.describe(both, k, at)}")
    assert np.array_equal(t["w_4"][:n].cpu().numpy().view(np.uint64), exp["w_4"])
    cols = dev.device_columns()
    for wname in ("w_l", "w_r", "w_o"):
        w = getattr(cols, wname)[:n]
        e, got = cols.var_values[w], t[wname + "_value"][:n]
        if not torch.equal(got, e):
            at = int((got != e).any(dim=1).nonzero()[0])
            raise AssertionError(f"{wname}_value differs first at row {at} (Variable {int(w[at])}): {ap.describe(both, wname, at)}")
    assert torch.equal(t["w_4_value"][:n], cols.var_values[t["w_4"][:n]])
    del cols
    for size in (1 << (n - 1).bit_length(), n):
        buf = torch.full((4 * size + GUARD_ROWS,), cv.CANARY, dtype=torch.int64, device="cuda:0")
        assert dev._lib.pg_composer_permutation(dev._h, size, buf.data_ptr()) == 0
        dev.sync()
        torch.cuda.synchronize()
        assert bool((buf[4 * size:] == cv.CANARY).all()), f"sigma at {size}: written past its end"
        wp.assert_sigma_equal(buf[:4 * size].view(4, size).cpu().numpy().view(np.uint64), ora.sigma(size), f"guarded, at {size}")


@pytest.mark.parametrize("kind", ap.KINDS, ids=repr)
def test_alignment_sweep(engine, kind):
    _, plan = ap.replay_on_oracle(kind, WITNESSES)      # the sizes of every call, for the room asserted before it
    dev = pg.StandardComposer(engine, *ap.CAPACITY[kind.name])      # fixed capacity: auto_grow stays off
    views = cv.CapacityViews(dev)
    both = ap.run_program(kind, dev, WITNESSES, ap.DeviceGuard(dev, views, plan))
    assert dev.capacity() == ap.CAPACITY[kind.name]

    # 1. the whole circuit against the oracle
    assert_whole_circuit(both)

    # 2. the values-only refresh: the same program, pads included, on other witnesses and against a second oracle
    n = dev.circuit_size()
    dev.sync()
    before = {k: views.rows[k][:n].clone() for k in ROW_COLS}
    dev.clear_witness()
    other = ap.run_program(kind, dev, OTHER_WITNESSES, ap.DeviceGuard(dev, views, plan, keep_rows=n))
    dev.sync()
    rows = n - 3        # (StandardComposer::new()'s three rows are not appended again)
    in_place, rewritten, refreshing = dev.refresh_stats()
    if kind.refreshed:
        assert (in_place, rewritten, refreshing) == (rows, 0, True), (kind.name, in_place, rewritten, refreshing)
    else:
        # "found in place only when no item fails, in either build ... The first append that differs from the previous build ends the
        # refresh: from there on everything is emitted in full" (pg_composer_clear_witness): the first batch with a failing item is
        # the first batch of 3, and it ends the refresh
        first_failing = next(n0 for what, n0, *_ in both.calls if "batch 3 " in what)
        assert (in_place, rewritten, refreshing) == (first_failing - 3, n - first_failing, False), (kind.name, in_place, rewritten)
    assert dev.circuit_size() == n
    for k in ROW_COLS:
        assert torch.equal(views.rows[k][:n], before[k]), f"{k} changed in the refresh"
    got, exp = dev.export()["var_values"], other.ora.export()["var_values"]
    if not np.array_equal(got, exp):
        at = int(np.argwhere((got != exp).any(axis=1))[0])
        raise AssertionError(f"after the refresh var_values differs from the second oracle's first at {at}: "
                             f"{ap.describe(other, 'var_values', at)}")
    assert dev.check() == other.first_bad()

    # 3. the f-rows into guarded outputs
    assert_f_rows_guarded(other)
    dev.close()
