"""Host-side handle on the gfx950 engine: owns a pg_engine, allocates output columns as torch tensors (device
memory + streams are torch's; nothing else of torch is used) and launches the batched gadgets through the C ABI."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from .scalar import BlsScalar


# [DEP-RECALL] dusk-plonk 0.8's coset constants (1, K1, K2, K3), one per wire in sigma's order (left, right, output, fourth)
DEFAULT_K = (1, 7, 13, 17)
# [DEP-RECALL] dusk-bls12_381's GENERATOR: the coset generator g of dusk-plonk 0.8's EvaluationDomain::coset_fft / coset_ifft
DEFAULT_COSET_GENERATOR = 7
# pg_ntt's kinds (include/plonk_gadgets_hip.h)
NTT_KINDS = {"fft": 0, "ifft": 1, "coset_fft": 2, "coset_ifft": 3}


def domain_generator(log2_n: int) -> BlsScalar:
    """omega of the 2^log2_n subgroup (log2_n <= 32): ROOT_OF_UNITY^(2^(32 - log2_n)), ROOT_OF_UNITY = 7^((q - 1) / 2^32)"""
    out = _lib.Scalar()
    st = _lib.load().pg_domain_generator(log2_n, C.byref(out))
    if st != 0:
        raise PgError(st, "pg_domain_generator")
    return BlsScalar(out)


def _field(x) -> BlsScalar:
    return x if isinstance(x, BlsScalar) else BlsScalar.from_int(int(x))


class PgError(RuntimeError):
    def __init__(self, status: int, where: str):
        lib = _lib.load()
        self.status = status
        super().__init__(f"{where}: {lib.pg_status_string(status).decode()} ({lib.pg_last_error().decode()})")


class NonExistingInverse(PgError):
    """Error::NonExistingInverse, /root/reference/src/errors.rs:17"""


@dataclass
class Layout:
    num_bits: int
    gates_per_item: int
    vars_per_item: int
    n_gates: int
    n_vars: int


@dataclass
class Columns:
    """The 8 live columns + variable table of a batch (device tensors, int64 storage of the u64 limbs/indices).
    Row r is gate gate_base + r; var_values[v] is Variable(var_base + v)."""
    q_m: torch.Tensor
    q_l: torch.Tensor
    q_r: torch.Tensor
    q_o: torch.Tensor
    q_c: torch.Tensor
    w_l: torch.Tensor
    w_r: torch.Tensor
    w_o: torch.Tensor
    var_values: torch.Tensor
    gate_base: int = 0
    var_base: int = 0
    slab: torch.Tensor | None = None  # allocate(spread_gib=...): the one allocation the nine arrays are views of

    SCALAR_COLS = ("q_m", "q_l", "q_r", "q_o", "q_c")
    WIRE_COLS = ("w_l", "w_r", "w_o")

    @staticmethod
    def allocate(n_gates: int, n_vars: int, device, gate_base: int = 0, var_base: int = 0, spread_gib: float = 0) -> "Columns":
        """spread_gib = 0: nine allocations, one after the other.
        spread_gib > 0: ONE allocation, the five selector columns spread_gib GiB apart, the wire columns and the variable
        table behind the last.  The emitters write the same row of all five selector columns at once; on MI355X five such streams
        inside one stretch of a few GiB of physical memory run 10-15 % slower than five streams tens of GiB apart (the 12-high
        stacks' ranks lie one after the other in the address space: streams in one rank share its banks).  A circuit of a few
        GB therefore does better in a slab that spans much of the card (C3: 0.575 -> 0.50 ms per step with the columns 16 GiB
        and more apart, tools/placement_sweep.py); columns of tens of GB each lie that far apart anyway.  The memory between the
        arrays belongs to the slab: the caller's to use for whatever else it streams (Columns.slab), or the price of the layout."""
        if spread_gib <= 0:
            sc = [torch.empty((n_gates, 4), dtype=torch.int64, device=device) for _ in range(5)]
            wc = [torch.empty((n_gates,), dtype=torch.int64, device=device) for _ in range(3)]
            vv = torch.empty((n_vars, 4), dtype=torch.int64, device=device)
            return Columns(*sc, *wc, vv, gate_base, var_base)
        # q_m q_l q_r q_o q_c a stride apart, then w_l w_r w_o var_values back to back behind q_c (of the layouts measured --
        # the others between the selector columns, before them, a stride apart themselves -- the best: tools/placement_policy.py);
        # the arithmetic is the library's (pg_columns_slab_layout: what a caller of the C ABI uses for its own block)
        off = (C.c_uint64 * 9)()
        total = C.c_uint64()
        st = _lib.load().pg_columns_slab_layout(n_gates, n_vars, int(spread_gib * (1 << 30)), off, C.byref(total))
        if st != 0:
            raise PgError(st, "pg_columns_slab_layout")
        align = 2 << 20
        slab = torch.empty(((total.value + align) // 8,), dtype=torch.int64, device=device)
        first = ((-slab.data_ptr()) % align) // 8
        at = [first + o // 8 for o in off]
        sel = [slab[at[c]:at[c] + n_gates * 4].view(n_gates, 4) for c in range(5)]
        wc = [slab[at[5 + c]:at[5 + c] + n_gates] for c in range(3)]
        vv = slab[at[8]:at[8] + n_vars * 4].view(n_vars, 4)
        cols = Columns(*sel, *wc, vv, gate_base, var_base)
        cols.slab = slab
        return cols

    def as_c(self) -> _lib.ColumnsC:
        return _lib.ColumnsC(*[getattr(self, n).data_ptr() for n in
                               ("q_m", "q_l", "q_r", "q_o", "q_c", "w_l", "w_r", "w_o", "var_values")])

    def nbytes(self) -> int:
        return sum(getattr(self, n).numel() * 8 for n in self.SCALAR_COLS + self.WIRE_COLS + ("var_values",))

    def to_numpy(self) -> dict:
        import numpy as np
        return {n: getattr(self, n).cpu().numpy().view(np.uint64)
                for n in self.SCALAR_COLS + self.WIRE_COLS + ("var_values",)}


class Engine:
    """pg_engine: one per GPU per host thread."""

    def __init__(self, device: int | torch.device | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("plonk_gadgets_amd needs a gfx950 GPU: there is no CPU path")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._lib = _lib.load()
        torch.cuda.init()
        h = C.c_void_p()
        st = self._lib.pg_engine_create(self.device.index or 0, C.byref(h))
        if st != 0:
            raise PgError(st, "pg_engine_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pg_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- range_check ---------------------------------------------------
    def range_check_layout(self, min_range: BlsScalar, max_range: BlsScalar, batch: int) -> Layout:
        lay = _lib.LayoutC()
        st = self._lib.pg_range_check_layout(C.byref(min_range.c), C.byref(max_range.c), batch, C.byref(lay))
        if st != 0:
            raise PgError(st, "pg_range_check_layout")
        return Layout(*[int(getattr(lay, f)) for f in ("num_bits", "gates_per_item", "vars_per_item", "n_gates", "n_vars")])

    def range_check_batch(self, min_range: BlsScalar, max_range: BlsScalar, witness: torch.Tensor,
                          gate_base: int = 0, var_base: int = 0, out: Columns | None = None,
                          result_vars: torch.Tensor | None = None, want_result_vars: bool = True):
        """for each witness: AllocatedScalar::allocate + range_check (/root/reference/src/range.rs:27-43).
        witness: int64[batch, 4] device tensor of Montgomery limbs.  Returns (Columns, result_vars)."""
        assert witness.is_cuda and witness.dtype == torch.int64 and witness.dim() == 2 and witness.shape[1] == 4
        assert witness.is_contiguous()
        batch = witness.shape[0]
        lay = self.range_check_layout(min_range, max_range, batch)
        if out is None:
            out = Columns.allocate(lay.n_gates, lay.n_vars, self.device, gate_base, var_base)
        if result_vars is None and want_result_vars:
            result_vars = torch.empty((batch,), dtype=torch.int64, device=self.device)
        cols = out.as_c()
        st = self._lib.pg_range_check_batch(self._h, C.byref(min_range.c), C.byref(max_range.c), witness.data_ptr(),
                                            batch, gate_base, var_base, C.byref(cols),
                                            result_vars.data_ptr() if result_vars is not None else None, self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_batch")
        return out, result_vars

    def range_check_sharded_batch(self, min_range: BlsScalar, max_range: BlsScalar, witness_local: torch.Tensor, total: int,
                                  rank: int, world: int, gate_base: int = 0, var_base: int = 0, out: Columns | None = None,
                                  result_vars: torch.Tensor | None = None):
        """this rank's shard of a `total`-item range_check batch, emitted at its global numbering
        (pg_range_check_sharded_batch; no communication).  Returns (Columns, result_vars)."""
        self._check_scalars(witness_local)
        shard = _lib.ShardC()
        st = self._lib.pg_range_check_shard_layout(C.byref(min_range.c), C.byref(max_range.c), total, rank, world, gate_base,
                                                   var_base, C.byref(shard))
        if st != 0:
            raise PgError(st, "pg_range_check_shard_layout")
        assert witness_local.shape[0] == shard.hi - shard.lo, (witness_local.shape, shard.lo, shard.hi)
        if out is None:
            out = Columns.allocate(shard.n_gates, shard.n_vars, self.device, shard.gate_base, shard.var_base)
        if result_vars is None:
            result_vars = torch.empty((witness_local.shape[0],), dtype=torch.int64, device=self.device)
        cols = out.as_c()
        st = self._lib.pg_range_check_sharded_batch(self._h, C.byref(min_range.c), C.byref(max_range.c), witness_local.data_ptr(),
                                                    total, rank, world, gate_base, var_base, C.byref(cols),
                                                    result_vars.data_ptr(), C.byref(shard), self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_sharded_batch")
        return out, result_vars

    # ---- encodings ------------------------------------------------------------------
    def scalars_from_canonical(self, raw: torch.Tensor):
        """int64[batch, 4] canonical little-endian values (BlsScalar::to_bytes) -> (Montgomery limbs, bad mask, bad count);
        values >= q come out as 0 and are flagged (BlsScalar::from_bytes would return Err)"""
        assert raw.is_cuda and raw.dtype == torch.int64 and raw.dim() == 2 and raw.shape[1] == 4 and raw.is_contiguous()
        out = torch.empty_like(raw)
        bad = torch.zeros((raw.shape[0],), dtype=torch.uint8, device=raw.device)
        n = C.c_uint64()
        st = self._lib.pg_scalars_from_canonical_batch(self._h, raw.data_ptr(), raw.shape[0], out.data_ptr(), bad.data_ptr(),
                                                       C.byref(n), self._stream())
        if st not in (0, 6):  # 6 = PG_ERR_BAD_ENCODING: flagged items, reported through the mask and the count
            raise PgError(st, "pg_scalars_from_canonical_batch")
        return out, bad, int(n.value)

    def scalars_to_canonical(self, scalars: torch.Tensor) -> torch.Tensor:
        assert scalars.is_cuda and scalars.dtype == torch.int64 and scalars.dim() == 2 and scalars.shape[1] == 4
        assert scalars.is_contiguous()
        out = torch.empty_like(scalars)
        st = self._lib.pg_scalars_to_canonical_batch(self._h, scalars.data_ptr(), scalars.shape[0], out.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_scalars_to_canonical_batch")
        return out

    def range_check_structure_batch(self, min_range: BlsScalar, max_range: BlsScalar, batch: int, gate_base: int,
                                    var_base: int, out: Columns):
        """selectors and wire indices of range_check_batch's rows -- no witnesses, `out.var_values` is left alone"""
        cols = out.as_c()
        st = self._lib.pg_range_check_structure_batch(self._h, C.byref(min_range.c), C.byref(max_range.c), batch, gate_base,
                                                      var_base, C.byref(cols), self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_structure_batch")
        return out

    # ---- helpers -------------------------------------------------------------
    def _layout(self, lay: "_lib.LayoutC") -> Layout:
        return Layout(*[int(getattr(lay, f)) for f in ("num_bits", "gates_per_item", "vars_per_item", "n_gates", "n_vars")])

    @staticmethod
    def _check_scalars(t: torch.Tensor, batch: int | None = None):
        assert t.is_cuda and t.dtype == torch.int64 and t.dim() == 2 and t.shape[1] == 4 and t.is_contiguous()
        assert batch is None or t.shape[0] == batch

    @staticmethod
    def _check_vars(t: torch.Tensor, batch: int):
        assert t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and t.shape[0] == batch and t.is_contiguous()

    def _out(self, out, n_gates, n_vars, gate_base, var_base):
        return out if out is not None else Columns.allocate(n_gates, n_vars, self.device, gate_base, var_base)

    # ---- max_bound -------------------------------------------------------------
    def max_bound_layout(self, max_range: BlsScalar, batch: int) -> Layout:
        lay = _lib.LayoutC()
        st = self._lib.pg_max_bound_layout(C.byref(max_range.c), batch, C.byref(lay))
        if st != 0:
            raise PgError(st, "pg_max_bound_layout")
        return self._layout(lay)

    def max_bound_batch(self, max_range: BlsScalar, witness: torch.Tensor, gate_base: int = 0, var_base: int = 0,
                        out: Columns | None = None):
        """for each witness: allocate + max_bound(composer, max_range, w) (/root/reference/src/range.rs:82-113).
        Returns (Columns, result_vars, num_bits)."""
        self._check_scalars(witness)
        batch = witness.shape[0]
        lay = self.max_bound_layout(max_range, batch)
        out = self._out(out, lay.n_gates, lay.n_vars, gate_base, var_base)
        res = torch.empty((batch,), dtype=torch.int64, device=self.device)
        cols = out.as_c()
        st = self._lib.pg_max_bound_batch(self._h, C.byref(max_range.c), witness.data_ptr(), batch, gate_base, var_base,
                                          C.byref(cols), res.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_batch")
        return out, res, lay.num_bits

    def max_bound_ragged_batch(self, max_range: torch.Tensor, witness: torch.Tensor, gate_base: int = 0,
                               var_base: int = 0):
        """one public bound PER ITEM (device tensor): plan (ladder bits + prefix sums on the device) then emit.
        Returns (Columns, result_vars, num_bits[int32 tensor], layout)."""
        self._check_scalars(witness)
        batch = witness.shape[0]
        self._check_scalars(max_range, batch)
        nb = torch.empty((batch,), dtype=torch.int32, device=self.device)
        roff = torch.empty((batch + 1,), dtype=torch.int64, device=self.device)
        voff = torch.empty((batch + 1,), dtype=torch.int64, device=self.device)
        lay = _lib.LayoutC()
        st = self._lib.pg_max_bound_ragged_plan(self._h, max_range.data_ptr(), batch, nb.data_ptr(), roff.data_ptr(),
                                                voff.data_ptr(), C.byref(lay), self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_ragged_plan")
        lay = self._layout(lay)
        out = Columns.allocate(lay.n_gates, lay.n_vars, self.device, gate_base, var_base)
        res = torch.empty((batch,), dtype=torch.int64, device=self.device)
        cols = out.as_c()
        st = self._lib.pg_max_bound_ragged_batch(self._h, max_range.data_ptr(), witness.data_ptr(), batch, nb.data_ptr(),
                                                 roff.data_ptr(), voff.data_ptr(), gate_base, var_base, C.byref(cols),
                                                 res.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_ragged_batch")
        return out, res, nb, lay

    # ---- range_check, one (min, max) pair per item ---------------------------------
    def _check_bound_arrays(self, min_range: torch.Tensor, max_range: torch.Tensor, witness: torch.Tensor) -> int:
        for t in (min_range, max_range, witness):
            self._check_scalars(t)
        if not (min_range.shape[0] == max_range.shape[0] == witness.shape[0]):
            raise ValueError(f"min_range, max_range and witness differ in length: {min_range.shape[0]}, {max_range.shape[0]}, "
                             f"{witness.shape[0]}")
        return witness.shape[0]

    def range_check_ragged_batch(self, min_range: torch.Tensor, max_range: torch.Tensor, witness: torch.Tensor,
                                 gate_base: int = 0, var_base: int = 0):
        """one public (min, max) pair PER ITEM (device tensors): for i { allocate(witness[i]); range_check(min[i], max[i], w) }
        -- plan (ladder bits from max + prefix sums on the device) then emit.
        Returns (Columns, result_vars, num_bits[int32 tensor], layout)."""
        batch = self._check_bound_arrays(min_range, max_range, witness)
        nb, roff, voff = self.ragged_buffers(batch)
        lay = self.range_check_ragged_plan(max_range, nb, roff, voff)
        out = Columns.allocate(lay.n_gates, lay.n_vars, self.device, gate_base, var_base)
        res = torch.empty((batch,), dtype=torch.int64, device=self.device)
        self.range_check_ragged_emit(min_range, max_range, witness, nb, roff, voff, out, res, gate_base, var_base)
        return out, res, nb, lay

    # ---- scalar gadgets ----------------------------------------------------------
    def _scalar2(self, fn_name, per_item, a_var, a_val, b_var, b_val, gate_base, var_base, out):
        batch = a_var.shape[0]
        self._check_vars(a_var, batch)
        self._check_vars(b_var, batch)
        self._check_scalars(a_val, batch)
        self._check_scalars(b_val, batch)
        out = self._out(out, per_item * batch, per_item * batch, gate_base, var_base)
        res = torch.empty((batch,), dtype=torch.int64, device=self.device)
        cols = out.as_c()
        st = getattr(self._lib, fn_name)(self._h, a_var.data_ptr(), a_val.data_ptr(), b_var.data_ptr(), b_val.data_ptr(),
                                         batch, gate_base, var_base, C.byref(cols), res.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, fn_name)
        return out, res

    def conditionally_select_zero_batch(self, x_var, x_val, select_var, select_val, gate_base=0, var_base=0, out=None):
        """/root/reference/src/scalar.rs:21-27, per item"""
        return self._scalar2("pg_conditionally_select_zero_batch", 1, x_var, x_val, select_var, select_val, gate_base,
                             var_base, out)

    def conditionally_select_one_batch(self, y_var, y_val, selector_var, selector_val, gate_base=0, var_base=0, out=None):
        """/root/reference/src/scalar.rs:36-59, per item"""
        return self._scalar2("pg_conditionally_select_one_batch", 4, y_var, y_val, selector_var, selector_val, gate_base,
                             var_base, out)

    def maybe_equal_batch(self, a_var, a_val, b_var, b_val, gate_base=0, var_base=0, out=None):
        """/root/reference/src/scalar.rs:105-140, per item"""
        return self._scalar2("pg_maybe_equal_batch", 3, a_var, a_val, b_var, b_val, gate_base, var_base, out)

    def _error_plan(self, fn_name, values, batch):
        roff = torch.empty((batch + 1,), dtype=torch.int64, device=self.device)
        voff = torch.empty((batch + 1,), dtype=torch.int64, device=self.device)
        err = torch.zeros((max(batch, 1),), dtype=torch.uint8, device=self.device)
        lay, nerr = _lib.LayoutC(), C.c_uint64()
        st = getattr(self._lib, fn_name)(self._h, values.data_ptr(), batch, roff.data_ptr(), voff.data_ptr(),
                                         err.data_ptr(), C.byref(lay), C.byref(nerr), self._stream())
        if st not in (0, 1):
            raise PgError(st, fn_name)
        return roff, voff, err[:batch], self._layout(lay), int(nerr.value)

    def is_non_zero_batch(self, var, value_assigned, gate_base=0, var_base=0, zero_var=0):
        """/root/reference/src/scalar.rs:63-97, per item.  Returns (Columns, err_mask[uint8], err_count): items whose
        value is 0 (Err(NonExistingInverse)) keep their partial emission (1 row, 1 variable)."""
        batch = var.shape[0]
        self._check_vars(var, batch)
        self._check_scalars(value_assigned, batch)
        roff, voff, err, lay, nerr = self._error_plan("pg_is_non_zero_plan", value_assigned, batch)
        out = Columns.allocate(lay.n_gates, lay.n_vars, self.device, gate_base, var_base)
        cols = out.as_c()
        st = self._lib.pg_is_non_zero_batch(self._h, var.data_ptr(), value_assigned.data_ptr(), batch, roff.data_ptr(),
                                            voff.data_ptr(), gate_base, var_base, zero_var, C.byref(cols), self._stream())
        if st != 0:
            raise PgError(st, "pg_is_non_zero_batch")
        return out, err, nerr

    def scalar_mix_batch(self, v, y, s, a, b, gate_base=0, var_base=0, zero_var=0):
        """BASELINE config 3, one launch: per item 5 x add_input, is_non_zero(v), conditionally_select_one(y, s),
        maybe_equal(a, b).  Returns (Columns, result_vars[batch,2], err_mask, err_count, layout)."""
        batch = v.shape[0]
        for t in (v, y, s, a, b):
            self._check_scalars(t, batch)
        roff, voff, err, lay, nerr = self._error_plan("pg_scalar_mix_plan", v, batch)
        out = Columns.allocate(lay.n_gates, lay.n_vars, self.device, gate_base, var_base)
        res = torch.empty((batch, 2), dtype=torch.int64, device=self.device)
        cols = out.as_c()
        st = self._lib.pg_scalar_mix_batch(self._h, v.data_ptr(), y.data_ptr(), s.data_ptr(), a.data_ptr(), b.data_ptr(),
                                           batch, roff.data_ptr(), voff.data_ptr(), gate_base, var_base, zero_var,
                                           C.byref(cols), res.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_scalar_mix_batch")
        return out, res, err, nerr, lay

    # ---- diagnostics -----------------------------------------------------------------
    def fill_columns(self, cols: "Columns", n_gates: int | None = None, n_vars: int | None = None, rows_per_tile: int = 0,
                     pattern: int = 0x0123456789ABCDEF):
        """pg_fill_columns: the emitters' store stream with nothing behind it, over these nine arrays (the store ceiling of
        a workload ON ITS OWN ARRAYS; bench.py times it beside every workload)"""
        n_gates = cols.q_m.shape[0] if n_gates is None else n_gates
        n_vars = cols.var_values.shape[0] if n_vars is None else n_vars
        cc = cols.as_c()
        st = self._lib.pg_fill_columns(self._h, C.byref(cc), n_gates, n_vars, rows_per_tile, pattern, self._stream())
        if st != 0:
            raise PgError(st, "pg_fill_columns")

    def fill_bytes(self, dst: torch.Tensor, streams: int = 5, pattern: int = 0x0123456789ABCDEF):
        """bare 16-B-per-lane streaming fill of `dst` as `streams` concurrent parts (the write ceiling bench.py quotes)"""
        nbytes = dst.numel() * dst.element_size()
        st = self._lib.pg_fill_bytes(self._h, dst.data_ptr(), nbytes, streams, pattern, self._stream())
        if st != 0:
            raise PgError(st, "pg_fill_bytes")

    # ---- gadgets on witnesses that are already allocated (the reference's exact argument: an AllocatedScalar) ----
    def range_check_allocated_batch(self, min_range: BlsScalar, max_range: BlsScalar, witness_var: torch.Tensor,
                                    witness: torch.Tensor, gate_base: int = 0, var_base: int = 0):
        """range_check(composer, min, max, AllocatedScalar{var, scalar}) per item: no allocate, 2n+523 variables"""
        self._check_scalars(witness)
        batch = witness.shape[0]
        self._check_vars(witness_var, batch)
        lay = self.range_check_layout(min_range, max_range, batch)
        out = Columns.allocate(lay.n_gates, lay.n_vars - batch, self.device, gate_base, var_base)
        res = torch.empty((batch,), dtype=torch.int64, device=self.device)
        cols = out.as_c()
        st = self._lib.pg_range_check_allocated_batch(self._h, C.byref(min_range.c), C.byref(max_range.c),
                                                      witness_var.data_ptr(), witness.data_ptr(), batch, gate_base,
                                                      var_base, C.byref(cols), res.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_allocated_batch")
        return out, res

    def max_bound_allocated_batch(self, max_range: BlsScalar, witness_var: torch.Tensor, witness: torch.Tensor,
                                  gate_base: int = 0, var_base: int = 0):
        self._check_scalars(witness)
        batch = witness.shape[0]
        self._check_vars(witness_var, batch)
        lay = self.max_bound_layout(max_range, batch)
        out = Columns.allocate(lay.n_gates, lay.n_vars - batch, self.device, gate_base, var_base)
        res = torch.empty((batch,), dtype=torch.int64, device=self.device)
        cols = out.as_c()
        st = self._lib.pg_max_bound_allocated_batch(self._h, C.byref(max_range.c), witness_var.data_ptr(),
                                                    witness.data_ptr(), batch, gate_base, var_base, C.byref(cols),
                                                    res.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_allocated_batch")
        return out, res, lay.num_bits

    def check_rows(self, cols: Columns, var_base: int | None = None, zero_var: int = 0) -> int:
        """every row of a self-contained batch satisfied?  -1, or the first failing row (device-side check)"""
        bad = C.c_int64()
        cc = cols.as_c()
        st = self._lib.pg_check_rows(self._h, C.byref(cc), cols.q_m.shape[0], cols.var_base if var_base is None else var_base,
                                     cols.var_values.shape[0], zero_var, C.byref(bad), self._stream())
        if st != 0:
            raise PgError(st, "pg_check_rows")
        return bad.value

    # ---- the copy permutation as field elements -------------------------------------------------------------
    def _domain(self, sigma: torch.Tensor, omega, k):
        assert sigma.is_cuda and sigma.dtype == torch.int64 and sigma.dim() == 2 and sigma.shape[0] == 4 and sigma.is_contiguous()
        padded_n = sigma.shape[1]
        if omega is None:
            assert padded_n > 0 and padded_n & (padded_n - 1) == 0, "padded_n must be a power of two"
            omega = domain_generator(padded_n.bit_length() - 1)
        ks = (_lib.Scalar * 4)(*[_field(x).c for x in k])
        return padded_n, _field(omega), ks

    def sigma_evaluations(self, sigma: torch.Tensor, omega=None, k=DEFAULT_K) -> torch.Tensor:
        """sigma (int64[4, padded_n], StandardComposer.permutation) -> its evaluations k[wire] * omega^gate as int64[4, padded_n, 4]
        (dusk-plonk's compute_permutation_lagrange); omega defaults to the generator of the padded_n subgroup"""
        padded_n, om, ks = self._domain(sigma, omega, k)
        out = torch.empty((4, padded_n, 4), dtype=torch.int64, device=self.device)
        st = self._lib.pg_sigma_evaluations(self._h, sigma.data_ptr(), padded_n, C.byref(om.c), ks, out.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_sigma_evaluations")
        return out

    def permutation_product(self, wire_values, sigma: torch.Tensor, beta, gamma, omega=None, k=DEFAULT_K, z_out=None):
        """PLONK's copy-permutation grand product -> (z int64[padded_n, 4], wrap BlsScalar): z[i] = prod_{r < i} num_r / den_r,
        wrap = the product of all padded_n ratios (one iff the wire values are constant on sigma's cycles); z_out: an
        int64[>= padded_n, 4] tensor whose first padded_n rows receive z (it is returned whole), else one is made.  wire_values: four
        int64[n_values, 4] tensors (the w_l / w_r / w_o / w_4 values of StandardComposer.materialize), rows >= n_values read as 0.
        Raises NonExistingInverse when a denominator is zero."""
        padded_n, om, ks = self._domain(sigma, omega, k)
        assert len(wire_values) == 4
        n_values = wire_values[0].shape[0]
        for w in wire_values:
            self._check_scalars(w, n_values)
        ptrs = (C.c_void_p * 4)(*[w.data_ptr() for w in wire_values])
        if z_out is None:
            z = torch.empty((padded_n, 4), dtype=torch.int64, device=self.device)
        else:
            z = z_out
            if not (self._rows(z) and z.dim() == 2 and z.shape[0] >= padded_n):
                raise ValueError(f"z_out must be int64[>= {padded_n}, 4] on the device with contiguous rows")
        wrap = torch.empty((1, 4), dtype=torch.int64, device=self.device)
        st = self._lib.pg_permutation_product(self._h, padded_n, ptrs, n_values, sigma.data_ptr(), C.byref(om.c), ks,
                                              C.byref(_field(beta).c), C.byref(_field(gamma).c), z.data_ptr(), wrap.data_ptr(),
                                              self._stream())
        if st == 1:
            raise NonExistingInverse(st, "pg_permutation_product")
        if st != 0:
            raise PgError(st, "pg_permutation_product")
        return z, BlsScalar.from_limbs([int(x) & (2**64 - 1) for x in wrap[0].tolist()])

    # ---- NTTs over the scalar field -----------------------------------------------------------------------------
    def _ntt(self, kind: str, x: torch.Tensor, log2_n, omega, g, inplace: bool) -> torch.Tensor:
        """x: int64[rows, 4] or int64[c, rows, 4] on the device (Montgomery limbs), rows <= 2^log2_n (log2_n defaults to the
        smallest that holds them).  Fewer rows are zero-padded into a new tensor; inplace=True transforms x itself (no padding
        allowed then: the point is to avoid the copy of a large column)."""
        assert x.is_cuda and x.dtype == torch.int64 and x.dim() in (2, 3) and x.shape[-1] == 4
        rows = x.shape[-2]
        if log2_n is None:
            log2_n = max(0, (rows - 1).bit_length())
        n = 1 << log2_n
        if rows > n:
            raise ValueError(f"{rows} rows do not fit a domain of 2^{log2_n} points")
        if inplace:
            if rows != n:
                raise ValueError("inplace=True needs exactly 2^log2_n rows: padding makes a new tensor")
            if x.stride(-1) != 1 or x.stride(-2) != 4 or (x.dim() == 3 and x.stride(0) % 4):
                raise ValueError("inplace=True needs rows of 4 contiguous limbs")
            y = x
        else:
            y = torch.zeros(x.shape[:-2] + (n, 4), dtype=torch.int64, device=self.device)
            y[..., :rows, :] = x
        cols = y.shape[0] if y.dim() == 3 else 1
        stride = y.stride(0) // 4 if cols > 1 else n  # (pg_ntt rejects a stride below n: overlapping columns)
        om = domain_generator(log2_n) if omega is None else _field(omega)
        coset = kind.startswith("coset")
        gp = C.byref(_field(g).c) if coset else None
        st = self._lib.pg_ntt(self._h, y.data_ptr(), cols, stride, log2_n, NTT_KINDS[kind], C.byref(om.c), gp, self._stream())
        if st != 0:
            raise PgError(st, "pg_ntt")
        return y

    def fft(self, x: torch.Tensor, log2_n=None, omega=None, g=DEFAULT_COSET_GENERATOR, inplace=False) -> torch.Tensor:
        """coefficients -> evaluations e_j = sum_i c_i omega^(ij) over the 2^log2_n subgroup (EvaluationDomain::fft); g is unused"""
        return self._ntt("fft", x, log2_n, omega, g, inplace)

    def ifft(self, x: torch.Tensor, log2_n=None, omega=None, g=DEFAULT_COSET_GENERATOR, inplace=False) -> torch.Tensor:
        """evaluations -> coefficients c_i = n^-1 sum_j e_j omega^(-ij) (EvaluationDomain::ifft); g is unused"""
        return self._ntt("ifft", x, log2_n, omega, g, inplace)

    def coset_fft(self, x: torch.Tensor, log2_n=None, omega=None, g=DEFAULT_COSET_GENERATOR, inplace=False) -> torch.Tensor:
        """coefficients -> evaluations over the coset g<omega>: fft(c_i g^i) (EvaluationDomain::coset_fft)"""
        return self._ntt("coset_fft", x, log2_n, omega, g, inplace)

    def coset_ifft(self, x: torch.Tensor, log2_n=None, omega=None, g=DEFAULT_COSET_GENERATOR, inplace=False) -> torch.Tensor:
        """the exact inverse of coset_fft: ifft, then times g^-i (EvaluationDomain::coset_ifft)"""
        return self._ntt("coset_ifft", x, log2_n, omega, g, inplace)

    # ---- the quotient polynomial and evaluations at a point ---------------------------------------------------
    QUOTIENT_SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith")

    @staticmethod
    def _rows(t: torch.Tensor) -> bool:
        """rows of 4 contiguous limbs on the device"""
        return t.is_cuda and t.dtype == torch.int64 and t.shape[-1] == 4 and t.stride(-1) == 1 and t.stride(-2) == 4

    def _quotient_call(self, blinded: bool, log2_n, p, q_range, alpha, beta, gamma, zeta, ks, g, out, scratch):
        """pg_quotient / pg_quotient_blinded, or pg_quotient_range when the range widget's selector polynomial is given"""
        n = 1 << log2_n
        args = (C.byref(_field(alpha).c), C.byref(_field(beta).c), C.byref(_field(gamma).c), C.byref(zeta.c), ks, C.byref(_field(g).c),
                out.data_ptr(), scratch.data_ptr(), self._stream())
        if q_range is None:
            name = "pg_quotient_blinded" if blinded else "pg_quotient"
            st = getattr(self._lib, name)(self._h, log2_n, C.byref(p), *args)
        else:
            if not (self._rows(q_range) and q_range.dim() == 2 and q_range.shape[0] == n):
                raise ValueError(f"q_range must be int64[{n}, 4] on the device with contiguous rows")
            name = "pg_quotient_range"
            st = self._lib.pg_quotient_range(self._h, log2_n, C.byref(p), q_range.data_ptr(), int(blinded), *args)
        if st != 0:
            raise PgError(st, name)
        return out

    def quotient(self, wires, z, sigmas, selectors: dict, pi=None, *, alpha, beta, gamma, omega_4n=None, k=DEFAULT_K,
                 g=DEFAULT_COSET_GENERATOR, scratch=None, q_range=None) -> torch.Tensor:
        """PLONK's quotient polynomial t (pg_quotient, the prover's round 3 for the arithmetic gate, the public inputs and the copy
        permutation) as int64[4, n, 4]: t_lo, t_mid, t_hi, t_4th.  Every input is a polynomial of n = 2^m coefficients
        (int64[n, 4] on the device; wires and sigmas: four of them, or int64[4, n, 4]); selectors: QUOTIENT_SELECTORS -> tensor;
        pi None is the zero polynomial.  omega_4n defaults to domain_generator(m + 2) (whose fourth power is the domain's omega);
        scratch: int64[PG_QUOTIENT_SCRATCH_COLS = 8, n, 4] the call may overwrite (allocated if None).
        StandardComposer.prover_polynomials() gives all of them.  q_range (int64[n, 4], None: none): the selector polynomial of the
        range widget, whose term joins N (pg_quotient_range)."""
        polys = [wires[j] for j in range(4)] + [z] + [sigmas[j] for j in range(4)] + [selectors[s] for s in self.QUOTIENT_SELECTORS]
        n = polys[0].shape[0]
        if n < 1 or n & (n - 1) or n > 1 << 30:
            raise ValueError(f"n = {n} must be a power of two <= 2^30")
        for t in polys + ([] if pi is None else [pi]):
            if not (self._rows(t) and t.dim() == 2 and t.shape[0] == n):
                raise ValueError(f"every input must be int64[{n}, 4] on the device with contiguous rows")
        log2_n = n.bit_length() - 1
        if scratch is None:
            scratch = torch.empty((8, n, 4), dtype=torch.int64, device=self.device)
        elif not (self._rows(scratch) and scratch.is_contiguous() and scratch.numel() >= 8 * n * 4):
            raise ValueError("scratch must be a contiguous int64 tensor of at least 8 x n x 4 elements")
        out = torch.empty((4, n, 4), dtype=torch.int64, device=self.device)
        p = _lib.QuotientPolysC()
        for j in range(4):
            p.w[j] = polys[j].data_ptr()
            p.sigma[j] = polys[5 + j].data_ptr()
        p.z = polys[4].data_ptr()
        for i, s in enumerate(self.QUOTIENT_SELECTORS):
            setattr(p, s, polys[9 + i].data_ptr())
        p.pi = None if pi is None else pi.data_ptr()
        zeta = domain_generator(log2_n + 2) if omega_4n is None else _field(omega_4n)
        ks = (_lib.Scalar * 4)(*[_field(x).c for x in k])
        return self._quotient_call(False, log2_n, p, q_range, alpha, beta, gamma, zeta, ks, g, out, scratch)

    def quotient_blinded(self, wires, z, sigmas, selectors: dict, pi=None, *, alpha, beta, gamma, omega_4n=None, k=DEFAULT_K,
                         g=DEFAULT_COSET_GENERATOR, scratch=None, q_range=None) -> torch.Tensor:
        """the quotient polynomial of BLINDED wire and permutation polynomials (pg_quotient_blinded) as one
        int64[4n + 8, 4]: the prover's parts are the views [0:n], [n:2n], [2n:3n] and [3n:4n + 8] (t_4th has n + 8 rows, the last
        one zero).  wires: int64[4, n + 2, 4] or four int64[n + 2, 4] (views of longer columns will do), z: int64[n + 3, 4], blinded
        as blind() blinds them; everything else as for quotient() (q_range, of n rows, included), n = 2^m >= 8 the length of the
        sigmas."""
        polys = [wires[j] for j in range(4)] + [z] + [sigmas[j] for j in range(4)] + [selectors[s] for s in self.QUOTIENT_SELECTORS]
        n = polys[5].shape[0]
        if n < 8 or n & (n - 1) or n > 1 << 30:
            raise ValueError(f"n = {n} must be a power of two from 2^3 to 2^30")
        for i, t in enumerate(polys + ([] if pi is None else [pi])):
            rows = n + (2 if i < 4 else 3 if i == 4 else 0)
            if not (self._rows(t) and t.dim() == 2 and t.shape[0] == rows):
                raise ValueError(f"the wires must be int64[{n + 2}, 4], z int64[{n + 3}, 4] and every other input int64[{n}, 4], on "
                                 "the device with contiguous rows")
        log2_n = n.bit_length() - 1
        if scratch is None:
            scratch = torch.empty((8, n, 4), dtype=torch.int64, device=self.device)
        elif not (self._rows(scratch) and scratch.is_contiguous() and scratch.numel() >= 8 * n * 4):
            raise ValueError("scratch must be a contiguous int64 tensor of at least 8 x n x 4 elements")
        out = torch.empty((4 * n + 8, 4), dtype=torch.int64, device=self.device)
        p = _lib.QuotientPolysC()
        for j in range(4):
            p.w[j] = polys[j].data_ptr()
            p.sigma[j] = polys[5 + j].data_ptr()
        p.z = polys[4].data_ptr()
        for i, s in enumerate(self.QUOTIENT_SELECTORS):
            setattr(p, s, polys[9 + i].data_ptr())
        p.pi = None if pi is None else pi.data_ptr()
        zeta = domain_generator(log2_n + 2) if omega_4n is None else _field(omega_4n)
        ks = (_lib.Scalar * 4)(*[_field(x).c for x in k])
        return self._quotient_call(True, log2_n, p, q_range, alpha, beta, gamma, zeta, ks, g, out, scratch)

    def blind(self, poly_ext: torch.Tensor, n: int, blinders) -> torch.Tensor:
        """poly_ext: int64[>= n + len(blinders), 4] on the device, rows 0..n-1 an interpolated polynomial and the rows behind them
        zero; blinders: two (a wire: b1, b0) or three (z: b2, b1, b0) scalars, highest power first.  In place, poly_ext becomes
        p + (sum_k b_k X^k)(X^n - 1): rows n.. get the blinders and the low rows lose them (4 rows change for a wire, 6 for z:
        through the host).  The values on the n-point domain do not change.  Returns poly_ext."""
        b = [_field(x) for x in reversed(list(blinders))]  # b0, b1, ...
        c = len(b)
        if not (self._rows(poly_ext) and poly_ext.dim() == 2 and n >= c and poly_ext.shape[0] >= n + c):
            raise ValueError(f"poly_ext must be int64[>= n + {c}, 4] on the device with contiguous rows")
        low = poly_ext[:c].cpu().tolist()
        rows = [(BlsScalar.from_limbs([int(x) & (2**64 - 1) for x in r]) - bi).limbs() for r, bi in zip(low, b)]
        signed = lambda limbs: [x - (1 << 64) if x >> 63 else x for x in limbs]
        poly_ext[:c] = torch.tensor([signed(r) for r in rows], dtype=torch.int64).to(self.device)
        poly_ext[n:n + c] = torch.tensor([signed(bi.limbs()) for bi in b], dtype=torch.int64).to(self.device)
        return poly_ext

    def evaluate(self, polys: torch.Tensor, point) -> list:
        """the polynomials at a point (pg_poly_evaluate, the prover's round 4): polys int64[n, 4] or int64[c, n, 4] coefficients
        on the device (rows of 4 contiguous limbs; n any size >= 1) -> c BlsScalars sum_i p_i point^i"""
        if not (self._rows(polys) and polys.dim() in (2, 3)):
            raise ValueError("polys must be int64[n, 4] or int64[c, n, 4] on the device with contiguous rows")
        cols = polys.shape[0] if polys.dim() == 3 else 1
        n = polys.shape[-2]
        stride = polys.stride(0) // 4 if polys.dim() == 3 and cols > 1 else n
        if polys.dim() == 3 and cols > 1 and polys.stride(0) % 4:
            raise ValueError("the columns of polys must start on whole rows")
        out = torch.empty((cols, 4), dtype=torch.int64, device=self.device)
        st = self._lib.pg_poly_evaluate(self._h, polys.data_ptr(), cols, stride, n, C.byref(_field(point).c), out.data_ptr(),
                                        self._stream())
        if st != 0:
            raise PgError(st, "pg_poly_evaluate")
        return [BlsScalar.from_limbs([int(x) & (2**64 - 1) for x in row]) for row in out.cpu().tolist()]

    # ---- openings: the prover's round 5 ---------------------------------------------------------------------------
    def _columns(self, polys, mu):
        """polys (a list of int64[n, 4] device tensors, or int64[c, n, 4]) and their weights -> (pointer array, weight array,
        c, n, the tensors kept alive)"""
        cols = list(polys.unbind(0)) if isinstance(polys, torch.Tensor) and polys.dim() == 3 else list(polys)
        if not cols:
            raise ValueError("no columns")
        n = cols[0].shape[0]
        for t in cols:
            if not (self._rows(t) and t.dim() == 2 and t.shape[0] == n):
                raise ValueError(f"every column must be int64[{n}, 4] on the device with contiguous rows")
        mu = list(mu)
        if len(mu) != len(cols):
            raise ValueError(f"{len(mu)} weights for {len(cols)} columns")
        ptrs = (C.c_void_p * len(cols))(*[t.data_ptr() for t in cols])
        ws = (_lib.Scalar * len(cols))(*[_field(m).c for m in mu])
        return ptrs, ws, len(cols), n, cols

    def open(self, polys, mu, point):
        """the KZG opening of f = sum_j mu_j p_j at `point` (pg_poly_open: CommitKey::compute_aggregate_witness then
        Polynomial::ruffini) -> (witness int64[n, 4], f(point) as a BlsScalar): f = witness (X - point) + f(point), the witness's
        top coefficient 0.  polys: up to 32 int64[n, 4] device tensors (they may repeat) or an int64[c, n, 4] tensor."""
        ptrs, ws, c, n, keep = self._columns(polys, mu)
        w = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        v = torch.empty((1, 4), dtype=torch.int64, device=self.device)
        st = self._lib.pg_poly_open(self._h, ptrs, ws, c, n, C.byref(_field(point).c), w.data_ptr(), v.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_poly_open")
        return w, BlsScalar.from_limbs([int(x) & (2**64 - 1) for x in v[0].tolist()])

    def combine(self, polys, mu) -> torch.Tensor:
        """sum_j mu_j p_j as int64[n, 4] (pg_poly_combine); polys as for open"""
        ptrs, ws, c, n, keep = self._columns(polys, mu)
        out = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        st = self._lib.pg_poly_combine(self._h, ptrs, ws, c, n, out.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_poly_combine")
        return out

    def msm(self, bases: torch.Tensor, scalars: torch.Tensor) -> list:
        """sum_i s_i P_i (pg_msm): bases int64[n, 12] (pg_g1_affine rows on the device), scalars int64[n, 4] or int64[c, n, 4]
        (Montgomery form, rows of 4 contiguous limbs, the columns at any whole-row stride) -> c G1Affines"""
        from .g1 import points_of
        if not (bases.dim() == 2 and bases.shape[1] == 12 and bases.dtype == torch.int64 and bases.device == self.device
                and bases.is_contiguous()):
            raise ValueError("bases must be a contiguous int64[n, 12] tensor on the engine's device")
        if not (self._rows(scalars) and scalars.dim() in (2, 3)):
            raise ValueError("scalars must be int64[n, 4] or int64[c, n, 4] on the device with contiguous rows")
        cols = scalars.shape[0] if scalars.dim() == 3 else 1
        n = scalars.shape[-2]
        if n != bases.shape[0]:
            raise ValueError(f"{n} scalars per column for {bases.shape[0]} bases")
        stride = scalars.stride(0) // 4 if scalars.dim() == 3 and cols > 1 else n
        if scalars.dim() == 3 and cols > 1 and scalars.stride(0) % 4:
            raise ValueError("the columns of scalars must start on whole rows")
        out = torch.empty((cols, 12), dtype=torch.int64, device=self.device)
        st = self._lib.pg_msm(self._h, bases.data_ptr(), scalars.data_ptr(), n, cols, stride, out.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_msm")
        return points_of(out)

    def msm_segmented(self, bases: torch.Tensor, scalars: torch.Tensor, offsets) -> torch.Tensor:
        """many small sums in one call (pg_msm_segmented): bases and scalars as for msm; offsets a Python sequence or a CPU
        int64 tensor of n_segs + 1 non-decreasing row offsets from 0 to n -> int64[n_segs, c, 12] on the device, row [s, j] the
        normalised sum of column j over the rows offsets[s] .. offsets[s + 1] - 1 ((0, 0) for an empty segment)"""
        if not (bases.dim() == 2 and bases.shape[1] == 12 and bases.dtype == torch.int64 and bases.device == self.device
                and bases.is_contiguous()):
            raise ValueError("bases must be a contiguous int64[n, 12] tensor on the engine's device")
        if not (self._rows(scalars) and scalars.dim() in (2, 3)):
            raise ValueError("scalars must be int64[n, 4] or int64[c, n, 4] on the device with contiguous rows")
        cols = scalars.shape[0] if scalars.dim() == 3 else 1
        n = scalars.shape[-2]
        if n != bases.shape[0]:
            raise ValueError(f"{n} scalars per column for {bases.shape[0]} bases")
        stride = scalars.stride(0) // 4 if scalars.dim() == 3 and cols > 1 else n
        if scalars.dim() == 3 and cols > 1 and scalars.stride(0) % 4:
            raise ValueError("the columns of scalars must start on whole rows")
        if isinstance(offsets, torch.Tensor):
            if not (offsets.dim() == 1 and offsets.dtype == torch.int64 and offsets.device.type == "cpu"):
                raise ValueError("offsets must be a Python sequence or a one-dimensional CPU int64 tensor")
            offsets = offsets.tolist()
        offsets = [int(x) for x in offsets]
        if not offsets or any(x < 0 for x in offsets):
            raise ValueError("offsets must hold n_segs + 1 non-negative row offsets")
        segs = len(offsets) - 1
        out = torch.empty((segs, cols, 12), dtype=torch.int64, device=self.device)
        st = self._lib.pg_msm_segmented(self._h, bases.data_ptr(), scalars.data_ptr(), n, cols, stride,
                                        (C.c_uint64 * len(offsets))(*offsets), segs, out.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_msm_segmented")
        return out

    # ---- G1 ingestion (pg_g1_decompress, pg_g1_check, pg_g1_compress) --------------------------------------------
    def _g1_points(self, points: torch.Tensor) -> None:
        if not (points.dim() == 2 and points.shape[1] == 12 and points.dtype == torch.int64 and points.device == self.device
                and points.is_contiguous() and points.shape[0] > 0):
            raise ValueError("points must be a contiguous, non-empty int64[n, 12] tensor on the engine's device")

    def _g1_decompress_into(self, data: torch.Tensor, check_subgroup: bool, out: torch.Tensor):
        """data uint8[48 n] on the device -> (status uint8[n], first_bad int64[1]); the points go to out int64[n, 12]"""
        n = data.numel() // 48
        status = torch.empty((n,), dtype=torch.uint8, device=self.device)
        first_bad = torch.empty((1,), dtype=torch.int64, device=self.device)
        st = self._lib.pg_g1_decompress(self._h, data.data_ptr(), n, 1 if check_subgroup else 0, out.data_ptr(), status.data_ptr(),
                                        first_bad.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_g1_decompress")
        return status, first_bad

    def g1_decompress(self, data, check_subgroup: bool = True):
        """48-byte encodings -> (points int64[n, 12], status uint8[n]) on the device (pg_g1_decompress).  data: bytes, or a
        uint8 tensor of 48 n elements (any shape; a host tensor is uploaded).  status[i] is a PG_G1_* value (g1.G1_STATUS names
        them); a point whose status is not 0 is the identity.  With check_subgroup the order-r membership test runs too."""
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.numel() and data.numel() % 48 == 0):
            raise ValueError("data must be bytes or a uint8 tensor of 48 n > 0 elements")
        data = data.to(self.device).contiguous().view(-1)
        out = torch.empty((data.numel() // 48, 12), dtype=torch.int64, device=self.device)
        status, _ = self._g1_decompress_into(data, check_subgroup, out)
        return out, status

    def _g1_check(self, points: torch.Tensor):
        self._g1_points(points)
        n = points.shape[0]
        status = torch.empty((n,), dtype=torch.uint8, device=self.device)
        first_bad = torch.empty((1,), dtype=torch.int64, device=self.device)
        st = self._lib.pg_g1_check(self._h, points.data_ptr(), n, status.data_ptr(), first_bad.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_g1_check")
        return status, first_bad

    def g1_check(self, points: torch.Tensor) -> torch.Tensor:
        """status uint8[n] of points int64[n, 12] (pg_g1_check): 0 for a point with reduced limbs, on the curve and of order
        dividing r (the identity included), else the PG_G1_* value of the first test it fails"""
        return self._g1_check(points)[0]

    def g1_compress(self, points: torch.Tensor) -> torch.Tensor:
        """points int64[n, 12] -> their encodings uint8[n, 48] on the device (pg_g1_compress)"""
        self._g1_points(points)
        out = torch.empty((points.shape[0], 48), dtype=torch.uint8, device=self.device)
        st = self._lib.pg_g1_compress(self._h, points.data_ptr(), points.shape[0], out.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_g1_compress")
        return out

    # ---- the verifier's sides from proof bytes (pg_plonk_sides) ------------------------------------------------------
    def plonk_sides(self, proofs: torch.Tensor, keys: torch.Tensor, key_index: torch.Tensor | None = None,
                    pi_off: torch.Tensor | None = None, pi_rows: torch.Tensor | None = None, pi_vals: torch.Tensor | None = None,
                    col_stride: int | None = None, range_term: bool = False):
        """pg_plonk_sides, everything on the device: proofs uint8[n, 1040] (or flat), keys uint8[n_keys * 1392] (the records of
        VerifierKey.record back to back), key_index int32[n] or None (key 0 for all), the public inputs as CSR arrays pi_off
        int64[n + 1], pi_rows int64[k], pi_vals int64[k, 4] (Montgomery limbs) or None for none -> (bases int64[23 n, 12],
        scalars int64[2, col_stride, 4], status uint8[n], where uint8[n]): what msm_segmented takes with the offsets 23 i.  The
        verdict on proof i is status[i] == 0 AND its pairing check (a rejected proof's rows are identities and zeros).
        range_term: pg_plonk_range_sides -- keys uint8[n_keys * 1488], the records of VerifierKey.record(...,
        range_term=True), and 24 rows a proof, the last one the key's q_range with the range widget's coefficient: bases
        int64[24 n, 12], the offsets 24 i."""
        from .verifier import PROOF_BYTES, RANGE_SIDES_ROWS, SIDES_ROWS, VerifierKey
        record_size = VerifierKey.RANGE_RECORD_SIZE if range_term else VerifierKey.RECORD_SIZE
        name = "pg_plonk_range_sides" if range_term else "pg_plonk_sides"

        def ok(t, dtype, what):
            if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device and t.is_contiguous()):
                raise ValueError(f"{what} must be a contiguous {dtype} tensor on the engine's device")
        ok(proofs, torch.uint8, "proofs")
        ok(keys, torch.uint8, "keys")
        if proofs.numel() % PROOF_BYTES or keys.numel() % record_size:
            raise ValueError(f"proofs are {PROOF_BYTES} bytes each and key records {record_size}")
        n, n_keys = proofs.numel() // PROOF_BYTES, keys.numel() // record_size
        if key_index is not None:
            ok(key_index, torch.int32, "key_index")
            if key_index.numel() != n:
                raise ValueError("key_index holds one index per proof")
        if pi_off is not None and (pi_rows is None or pi_rows.numel() == 0):
            pi_off = pi_rows = pi_vals = None  # (no proof has a public input: the call takes no arrays then)
        if pi_off is not None:
            ok(pi_off, torch.int64, "pi_off")
            ok(pi_rows, torch.int64, "pi_rows")
            ok(pi_vals, torch.int64, "pi_vals")
            if pi_off.numel() != n + 1 or pi_vals.numel() != 4 * pi_rows.numel():
                raise ValueError("pi_off holds n + 1 offsets, pi_vals four limbs per row of pi_rows")
        rows = (RANGE_SIDES_ROWS if range_term else SIDES_ROWS) * n
        col_stride = rows if col_stride is None else int(col_stride)
        bases = torch.empty((rows, 12), dtype=torch.int64, device=self.device)
        scalars = torch.empty((2, col_stride, 4), dtype=torch.int64, device=self.device)
        status = torch.empty((n,), dtype=torch.uint8, device=self.device)
        where = torch.empty((n,), dtype=torch.uint8, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None
        st = getattr(self._lib, name)(self._h, proofs.data_ptr(), n, keys.data_ptr(), n_keys, ptr(key_index), ptr(pi_off), ptr(pi_rows),
                                      ptr(pi_vals), bases.data_ptr(), scalars.data_ptr(), col_stride, status.data_ptr(),
                                      where.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, name)
        return bases, scalars, status, where

    # ---- two-step forms of the ragged batches (plan once into caller-owned buffers, emit many times) ------------
    def ragged_buffers(self, batch: int):
        """(num_bits int32[batch], row_off int64[batch+1], var_off int64[batch+1]) for the *_plan calls"""
        return (torch.empty((batch,), dtype=torch.int32, device=self.device),
                torch.empty((batch + 1,), dtype=torch.int64, device=self.device),
                torch.empty((batch + 1,), dtype=torch.int64, device=self.device))

    def max_bound_ragged_plan(self, max_range: torch.Tensor, num_bits, row_off, var_off) -> Layout:
        lay = _lib.LayoutC()
        st = self._lib.pg_max_bound_ragged_plan(self._h, max_range.data_ptr(), max_range.shape[0], num_bits.data_ptr(),
                                                row_off.data_ptr(), var_off.data_ptr(), C.byref(lay), self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_ragged_plan")
        return self._layout(lay)

    def max_bound_ragged_emit(self, max_range, witness, num_bits, row_off, var_off, out: Columns, result_vars=None,
                              gate_base: int = 0, var_base: int = 0):
        cols = out.as_c()
        st = self._lib.pg_max_bound_ragged_batch(self._h, max_range.data_ptr(), witness.data_ptr(), witness.shape[0],
                                                 num_bits.data_ptr(), row_off.data_ptr(), var_off.data_ptr(), gate_base,
                                                 var_base, C.byref(cols),
                                                 result_vars.data_ptr() if result_vars is not None else None, self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_ragged_batch")

    def range_check_ragged_plan(self, max_range: torch.Tensor, num_bits, row_off, var_off) -> Layout:
        """ladder bits and prefix sums of range_check items from their upper bounds (min_bound reuses max's ladder length)"""
        lay = _lib.LayoutC()
        st = self._lib.pg_range_check_ragged_plan(self._h, max_range.data_ptr(), max_range.shape[0], num_bits.data_ptr(),
                                                  row_off.data_ptr(), var_off.data_ptr(), C.byref(lay), self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_ragged_plan")
        return self._layout(lay)

    def range_check_ragged_emit(self, min_range, max_range, witness, num_bits, row_off, var_off, out: Columns, result_vars=None,
                                gate_base: int = 0, var_base: int = 0):
        batch = self._check_bound_arrays(min_range, max_range, witness)
        cols = out.as_c()
        st = self._lib.pg_range_check_ragged_batch(self._h, min_range.data_ptr(), max_range.data_ptr(), witness.data_ptr(), batch,
                                                   num_bits.data_ptr(), row_off.data_ptr(), var_off.data_ptr(), gate_base,
                                                   var_base, C.byref(cols),
                                                   result_vars.data_ptr() if result_vars is not None else None, self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_ragged_batch")

    def scalar_mix_plan(self, v: torch.Tensor, row_off, var_off, err_mask=None):
        """-> (Layout, err_count); PG_ERR_NON_EXISTING_INVERSE is reported through err_count, not raised"""
        lay, nerr = _lib.LayoutC(), C.c_uint64()
        st = self._lib.pg_scalar_mix_plan(self._h, v.data_ptr(), v.shape[0], row_off.data_ptr(), var_off.data_ptr(),
                                          err_mask.data_ptr() if err_mask is not None else None, C.byref(lay),
                                          C.byref(nerr), self._stream())
        if st not in (0, 1):
            raise PgError(st, "pg_scalar_mix_plan")
        return self._layout(lay), int(nerr.value)

    def scalar_mix_emit(self, v, y, s, a, b, row_off, var_off, out: Columns, result_vars=None, gate_base: int = 0,
                        var_base: int = 0, zero_var: int = 0):
        cols = out.as_c()
        st = self._lib.pg_scalar_mix_batch(self._h, v.data_ptr(), y.data_ptr(), s.data_ptr(), a.data_ptr(), b.data_ptr(),
                                           v.shape[0], row_off.data_ptr(), var_off.data_ptr(), gate_base, var_base, zero_var,
                                           C.byref(cols), result_vars.data_ptr() if result_vars is not None else None,
                                           self._stream())
        if st != 0:
            raise PgError(st, "pg_scalar_mix_batch")

    def scalar_mix_planned(self, v, y, s, a, b, row_off, var_off, out: Columns, result_vars=None, err_mask=None,
                           gate_base: int = 0, var_base: int = 0, zero_var: int = 0):
        """plan + emit in one call (pg_scalar_mix_planned_batch): `out` must hold the worst case, 10 rows and 15 variables
        per item; the totals are read with plan_result() after a synchronisation"""
        cols = out.as_c()
        st = self._lib.pg_scalar_mix_planned_batch(self._h, v.data_ptr(), y.data_ptr(), s.data_ptr(), a.data_ptr(), b.data_ptr(),
                                                   v.shape[0], row_off.data_ptr(), var_off.data_ptr(),
                                                   err_mask.data_ptr() if err_mask is not None else None, gate_base, var_base,
                                                   zero_var, C.byref(cols),
                                                   result_vars.data_ptr() if result_vars is not None else None, self._stream())
        if st != 0:
            raise PgError(st, "pg_scalar_mix_planned_batch")

    # ---- witness refresh: the variable assignments of a call, no rows (pg_*_values_batch) ----------------------------------
    def range_check_values_batch(self, min_range: BlsScalar, max_range: BlsScalar, witness: torch.Tensor,
                                 var_values: torch.Tensor | None = None) -> torch.Tensor:
        """what range_check_batch writes into Columns.var_values, and nothing else: the same circuit rebuilt with other
        witnesses (prover.clear_witness() and the calls again, /root/reference/tests/scalar_gadgets_tests.rs:108-119)"""
        self._check_scalars(witness)
        batch = witness.shape[0]
        lay = self.range_check_layout(min_range, max_range, batch)
        if var_values is None:
            var_values = torch.empty((lay.n_vars, 4), dtype=torch.int64, device=self.device)
        assert var_values.is_contiguous() and var_values.shape == (lay.n_vars, 4)
        st = self._lib.pg_range_check_values_batch(self._h, C.byref(min_range.c), C.byref(max_range.c), witness.data_ptr(), batch,
                                                   var_values.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_values_batch")
        return var_values

    def max_bound_values_batch(self, max_range: BlsScalar, witness: torch.Tensor, var_values: torch.Tensor | None = None) -> torch.Tensor:
        self._check_scalars(witness)
        batch = witness.shape[0]
        lay = self.max_bound_layout(max_range, batch)
        if var_values is None:
            var_values = torch.empty((lay.n_vars, 4), dtype=torch.int64, device=self.device)
        assert var_values.is_contiguous() and var_values.shape == (lay.n_vars, 4)
        st = self._lib.pg_max_bound_values_batch(self._h, C.byref(max_range.c), witness.data_ptr(), batch, var_values.data_ptr(),
                                                 self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_values_batch")
        return var_values

    def max_bound_ragged_values(self, max_range, witness, num_bits, row_off, var_off, var_values: torch.Tensor):
        """the ragged call's assignments under the plan of its (public) bounds"""
        st = self._lib.pg_max_bound_ragged_values_batch(self._h, max_range.data_ptr(), witness.data_ptr(), witness.shape[0],
                                                        num_bits.data_ptr(), row_off.data_ptr(), var_off.data_ptr(),
                                                        var_values.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_ragged_values_batch")
        return var_values

    def range_check_ragged_values(self, min_range, max_range, witness, num_bits, row_off, var_off, var_values: torch.Tensor):
        """the ragged range_check's assignments under the plan of its (public) bounds"""
        batch = self._check_bound_arrays(min_range, max_range, witness)
        st = self._lib.pg_range_check_ragged_values_batch(self._h, min_range.data_ptr(), max_range.data_ptr(), witness.data_ptr(),
                                                          batch, num_bits.data_ptr(), row_off.data_ptr(), var_off.data_ptr(),
                                                          var_values.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_ragged_values_batch")
        return var_values

    def scalar_mix_values(self, v, y, s, a, b, row_off, var_off, var_values: torch.Tensor, err_mask=None):
        """the fused mix's assignments AND its plan for these witnesses (row_off / var_off / err_mask are outputs; totals:
        plan_result()): an item's shape depends on its witness, the caller compares the plan with the circuit it has"""
        st = self._lib.pg_scalar_mix_values_batch(self._h, v.data_ptr(), y.data_ptr(), s.data_ptr(), a.data_ptr(), b.data_ptr(),
                                                  v.shape[0], row_off.data_ptr(), var_off.data_ptr(),
                                                  err_mask.data_ptr() if err_mask is not None else None, var_values.data_ptr(),
                                                  self._stream())
        if st != 0:
            raise PgError(st, "pg_scalar_mix_values_batch")
        return var_values

    # ---- asynchronous plans (no host round trip between plan and emit; totals read back later) -----------------
    def max_bound_ragged_plan_async(self, max_range: torch.Tensor, num_bits, row_off, var_off):
        st = self._lib.pg_max_bound_ragged_plan_async(self._h, max_range.data_ptr(), max_range.shape[0], num_bits.data_ptr(),
                                                      row_off.data_ptr(), var_off.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_max_bound_ragged_plan_async")

    def range_check_ragged_plan_async(self, max_range: torch.Tensor, num_bits, row_off, var_off):
        st = self._lib.pg_range_check_ragged_plan_async(self._h, max_range.data_ptr(), max_range.shape[0], num_bits.data_ptr(),
                                                        row_off.data_ptr(), var_off.data_ptr(), self._stream())
        if st != 0:
            raise PgError(st, "pg_range_check_ragged_plan_async")

    def scalar_mix_plan_async(self, v: torch.Tensor, row_off, var_off, err_mask=None):
        st = self._lib.pg_scalar_mix_plan_async(self._h, v.data_ptr(), v.shape[0], row_off.data_ptr(), var_off.data_ptr(),
                                                err_mask.data_ptr() if err_mask is not None else None, self._stream())
        if st != 0:
            raise PgError(st, "pg_scalar_mix_plan_async")

    def plan_result(self):
        """(Layout, err_count) of the most recent plan; call after synchronising the stream it ran on"""
        lay, nerr = _lib.LayoutC(), C.c_uint64()
        st = self._lib.pg_plan_result(self._h, C.byref(lay), C.byref(nerr))
        if st not in (0, 1):
            raise PgError(st, "pg_plan_result")
        return self._layout(lay), int(nerr.value)
