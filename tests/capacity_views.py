"""TEST INFRASTRUCTURE: live tensors over the WHOLE capacity of a StandardComposer -- the five selector columns, the three wire columns
and the variable table, from pg_composer_columns' pointers (as StandardComposer.device_columns takes them) and
StandardComposer.capacity()'s sizes -- so that a test sees every store an append makes, not only those inside its own rows.

    views = CapacityViews(dev)
    armed = views.arm(dev)             # sync; canary behind the live part; the live part cloned
    ... one append (or a group of them) ...
    views.disarm(dev, armed, "what")   # sync; the old live part bit for bit unchanged, the canary intact behind the new end, and gone
                                       # from every row and Variable of the call itself

device_columns and export show rows [0, circuit_size) only: a store one row before a call is seen there only where check() trips on
it, a store into the spare capacity never.  Here the spare capacity holds 0x5A5A5A5A5A5A5A5A (the value of the suite's other canary
tests), and the rows and Variables that were live before the call are compared with their clone, on the device.

No column is left un-armed: neither the header nor csrc/composer.hpp promises anything of a column behind the live part (the composer
allocates its columns without clearing them), so every byte there is the test's to fill.

Two rules keep a wrong store inside the allocation, where it is a mismatch and not a wild address (tests/test_gpu_append_alignment.py):
the composer's capacity is fixed (never auto_grow, never reserve -- the columns would move away from the views), and room() is asserted
before every guarded call: at least ROOM_BEHIND rows and Variables of spare capacity behind the call's end and ROOM_BEFORE_ROWS rows /
ROOM_BEFORE_VARS Variables in front of its start.  A sweep that skips lanes to start on a 128-byte line can at worst store one such
skip too early or too late: 112 bytes of selectors, 14 wire rows, 3 Variables."""
import ctypes as C

import torch

from plonk_gadgets_amd import _lib
from plonk_gadgets_amd.engine import Columns

CANARY = 0x5A5A5A5A5A5A5A5A
ROOM_BEHIND = 64
ROOM_BEFORE_ROWS, ROOM_BEFORE_VARS = 16, 4
ROW_COLS = Columns.SCALAR_COLS + Columns.WIRE_COLS      # the eight row columns, in pg_columns' order


class _Mem:
    def __init__(self, ptr, words):
        self.__cuda_array_interface__ = {"shape": (words,), "typestr": "<i8", "data": (int(ptr), False), "version": 2}


def room(n_before, nv_before, n_after, nv_after, gate_capacity, var_capacity, what=""):
    """the two rules' second one, for a call that takes the composer from (n_before, nv_before) to (n_after, nv_after); plain
    integers, so the oracle-only replay of a program asserts it without a device"""
    assert n_before >= ROOM_BEFORE_ROWS and nv_before >= ROOM_BEFORE_VARS, \
        f"{what}: {n_before} rows / {nv_before} Variables in front of the call, {ROOM_BEFORE_ROWS} / {ROOM_BEFORE_VARS} wanted"
    assert gate_capacity - n_after >= ROOM_BEHIND and var_capacity - nv_after >= ROOM_BEHIND, \
        (f"{what}: {gate_capacity - n_after} rows / {var_capacity - nv_after} Variables of spare capacity behind the call, "
         f"{ROOM_BEHIND} wanted")


class Armed:
    """what arm() leaves for disarm(): the live sizes and the clone of the live part"""

    def __init__(self, n, nv, rows, variables):
        self.n, self.nv, self.rows, self.variables = n, nv, rows, variables


class CapacityViews:
    def __init__(self, dev):
        cc = _lib.ColumnsC()
        assert dev._lib.pg_composer_columns(dev._h, C.byref(cc)) == 0
        self.gate_capacity, self.var_capacity = dev.capacity()
        device = dev.engine.device

        def words(ptr, count):
            return torch.as_tensor(_Mem(ptr, count), device=device)
        g, v = self.gate_capacity, self.var_capacity
        self.rows = {k: words(getattr(cc, k), g * 4).view(g, 4) if k in Columns.SCALAR_COLS else words(getattr(cc, k), g) for k in ROW_COLS}
        self.variables = words(cc.var_values, v * 4).view(v, 4)

    def _same_place(self, dev):
        assert dev.capacity() == (self.gate_capacity, self.var_capacity), "the composer grew: the views are stale"

    def arm(self, dev, keep_rows=0):
        """keep_rows: rows [0, keep_rows) count as live whatever circuit_size() says -- after clear_witness the previous build's rows
        lie behind the composer's end and a values-only refresh relies on them: they are snapshotted, not overwritten, and disarm
        requires them unchanged (which is what "writes only its assignments" means for the call's own rows).  The Variables behind
        num_variables() get the canary either way: a refresh writes every assignment of its call again."""
        dev.sync()
        self._same_place(dev)
        n, nv = max(dev.circuit_size(), keep_rows), dev.num_variables()
        for col in self.rows.values():
            col[n:].fill_(CANARY)
        self.variables[nv:].fill_(CANARY)
        armed = Armed(n, nv, {k: col[:n].clone() for k, col in self.rows.items()}, self.variables[:nv].clone())
        torch.cuda.synchronize(dev.engine.device)   # the fills are in memory before any stream of the engine's writes
        return armed

    def disarm(self, dev, armed, what="", span=None):
        """`what` names the call in a failure (kind, target alignment, batch); span = ((first row, end row), (first Variable, end
        Variable)) of the call where that is not (armed size, size now): a refresh, whose rows lie inside the kept part"""
        dev.sync()
        self._same_place(dev)
        n, nv = max(dev.circuit_size(), armed.n), dev.num_variables()
        assert nv >= armed.nv
        (rf, re_), (vf, ve) = span if span is not None else ((armed.n, n), (armed.nv, nv))
        checks = []        # (column, unit, differs(), base, first, end, why), judged on the device and fetched as one verdict
        for k, col in self.rows.items():
            checks.append((k, "row", lambda col=col, k=k: col[:armed.n] != armed.rows[k], 0, rf, re_,
                           "was live before the call and changed"))
            checks.append((k, "row", lambda col=col: col[n:] != CANARY, n, rf, re_,
                           "lies behind the composer's end and lost its canary"))
            if n > armed.n:    # (a refresh appends no row behind the kept part)
                checks.append((k, "row", lambda col=col: self._still_canary(col[armed.n:n]), armed.n, rf, re_,
                               "is the call's own and was never written (it still holds the canary)"))
        checks.append(("var_values", "Variable", lambda: self._still_canary(self.variables[armed.nv:nv]), armed.nv, vf, ve,
                       "is the call's own and was never written (it still holds the canary)"))
        checks.append(("var_values", "Variable", lambda: self.variables[:armed.nv] != armed.variables, 0, vf, ve,
                       "was live before the call and changed"))
        checks.append(("var_values", "Variable", lambda: self.variables[nv:] != CANARY, nv, vf, ve,
                       "lies behind the composer's end and lost its canary"))
        verdict = torch.stack([c[2]().any() for c in checks])
        if bool(verdict.any()):
            for bad, (column, unit, differs, base, first, end, why) in zip(verdict.tolist(), checks):
                if bad:
                    self._report(what, column, unit, differs(), base, first, end, why)

    @staticmethod
    def _still_canary(part):
        """no selector, wire or assignment an append writes is the canary in every word (a wire is a Variable's number; a scalar of
        four such limbs would be one chosen to be)"""
        return (part == CANARY).all(dim=1) if part.dim() == 2 else part == CANARY

    @staticmethod
    def _report(what, column, unit, differs, base, first, end, why):
        if differs.dim() == 2:
            differs = differs.any(dim=1)
        where = differs.nonzero().flatten()
        at, last = base + int(where[0]), base + int(where[-1])
        place = (f"{first - at} before the call's first {unit}" if at < first else
                 f"{at - (end - 1)} behind the call's last {unit}" if at >= end else f"the call's own {unit} {at - first}")
        raise AssertionError(f"{what}: {column}: {unit} {at} {why} ({place}; the call's own are [{first}, {end}); "
                             f"{int(where.numel())} such, the last at {last})")
