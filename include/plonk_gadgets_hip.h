/*
 * plonk_gadgets_hip.h -- C ABI of libplonk_gadgets_hip.so, the MI355X (gfx950)
 * batched constraint-evaluation engine for the gadget hot path of
 * dusk-network/plonk_gadgets.
 *
 * The reference has no FFI of its own: it is a safe-Rust library whose whole
 * interface is six public gadget functions + `AllocatedScalar` + `Error`
 * (/root/reference/src/lib.rs:37-45), every one taking
 * `&mut StandardComposer`.  Each entry point below names the reference
 * function(s) it replaces; INTEGRATION.md shows the Rust `extern "C"` shim a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C types only; no HIP or torch types in any signature.
 *   - `pg_scalar` is bit-identical to BlsScalar's inner `[u64; 4]`
 *     (Montgomery limbs, little-endian, fully reduced).
 *   - pointers named `d_*` and every pointer inside `pg_columns` are DEVICE
 *     pointers on the engine's GPU; everything else is host memory.
 *     (Speed, not correctness: the emitters line their wave stores up with
 *     128-byte lines from the address of the FIRST array of each kind; arrays
 *     that all start on lines -- hipMalloc's do -- are written 11-17 % faster
 *     than arrays that start at different offsets inside a line.)
 *   - the caller allocates and frees every output buffer (sizes come from the
 *     `pg_*_layout` / `pg_*_plan` queries); the engine owns only its constant
 *     table and grow-only scratch (inverses of the current call, prefix-sum
 *     temporaries).  Because that scratch is per engine, calls on one engine
 *     must be issued on ONE stream at a time (one engine per stream/thread).
 *     A call on another stream than the previous one is ordered behind it by
 *     an event recorded on the previous stream: keep a stream alive until the
 *     next call on the engine has been issued (a stream that has been
 *     destroyed costs that call a device synchronisation instead).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     Batch calls enqueue and return; synchronise the stream (or call
 *     pg_engine_sync) before reading results.
 *   - every function returns a pg_status; nothing aborts.  Conditions on
 *     which the reference panics map to PG_ERR_INVALID_ARGUMENT.
 *   - an engine handle is not thread-safe (the reference is single-threaded
 *     per composer by its `&mut` borrow, e.g. src/range.rs:27-32): use one
 *     handle per host thread.
 */
#ifndef PLONK_GADGETS_HIP_H
#define PLONK_GADGETS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pg_status {
    PG_OK = 0,
    PG_ERR_NON_EXISTING_INVERSE = 1, /* Error::NonExistingInverse, src/errors.rs:17 (raised at src/scalar.rs:79) */
    PG_ERR_INVALID_ARGUMENT = 2,     /* NULL / misaligned pointer, num_bits > 256 (src/range.rs:134 panics), ... */
    PG_ERR_NO_DEVICE = 3,            /* no gfx950 device / HIP runtime failure at engine creation */
    PG_ERR_HIP = 4,                  /* a HIP call failed; pg_last_error() has the text */
    PG_ERR_CAPACITY = 5,             /* composer buffers too small for the append */
    PG_ERR_BAD_ENCODING = 6          /* pg_scalars_from_canonical_batch: some 32-byte encodings are >= q (BlsScalar::from_bytes -> Err) */
} pg_status;

typedef struct pg_scalar { uint64_t l[4]; } pg_scalar; /* BlsScalar */
typedef uint64_t pg_variable;                         /* Variable(usize) */

/* AllocatedScalar, src/allocated_scalar.rs:17-23.  The Rust struct has no
 * #[repr(C)]; a shim converts field by field. */
typedef struct pg_allocated_scalar {
    pg_variable var;
    pg_scalar scalar;
} pg_allocated_scalar;

/* The live columns a gate row occupies on this path (SURVEY.md section 8a row
 * a14) plus the variable-assignment table.  Row r of a batch call is gate
 * `gate_base + r`; entry v of var_values is Variable(var_base + v).  Every
 * row has q_4 = 0, q_arith = 1, the other selectors 0 and w_4 = zero_var;
 * those constant columns are not materialised here (pg_composer does). */
typedef struct pg_columns {
    pg_scalar *q_m, *q_l, *q_r, *q_o, *q_c; /* device, 16-byte aligned */
    uint64_t *w_l, *w_r, *w_o;              /* device, 8-byte aligned   */
    pg_scalar *var_values;                  /* device, 16-byte aligned */
} pg_columns;

typedef struct pg_layout {
    uint64_t num_bits;       /* ladder length n (0 for gadgets without a ladder / ragged batches) */
    uint64_t gates_per_item; /* rows one item emits (0 if ragged)      */
    uint64_t vars_per_item;  /* variables one item creates (0 if ragged) */
    uint64_t n_gates;        /* total rows of the batch                 */
    uint64_t n_vars;         /* total variables of the batch            */
} pg_layout;

typedef struct pg_engine pg_engine;

/* ---- engine ----------------------------------------------------------- */
pg_status pg_engine_create(int device, pg_engine **out);
void pg_engine_destroy(pg_engine *e);
pg_status pg_engine_sync(pg_engine *e, void *stream);
const char *pg_status_string(pg_status s);
const char *pg_last_error(void);
/* "gfx950" etc.; what the library was built for and what it runs on */
const char *pg_build_arch(void);

/* ---- BlsScalar helpers (host) ------------------------------------------
 * what a host needs to form the public arguments: BlsScalar::from(u64),
 * from_raw/to canonical, neg/sub/add/mul, and the two pure functions of
 * src/range.rs:173-189. */
void pg_scalar_from_u64(uint64_t v, pg_scalar *out);
void pg_scalar_from_canonical(const uint64_t raw[4], pg_scalar *out);
void pg_scalar_to_canonical(const pg_scalar *s, uint64_t raw[4]);
void pg_scalar_add(const pg_scalar *a, const pg_scalar *b, pg_scalar *out);
void pg_scalar_sub(const pg_scalar *a, const pg_scalar *b, pg_scalar *out);
void pg_scalar_neg(const pg_scalar *a, pg_scalar *out);
void pg_scalar_mul(const pg_scalar *a, const pg_scalar *b, pg_scalar *out);
/* BlsScalar::invert (used at src/scalar.rs:73,121): PG_ERR_NON_EXISTING_INVERSE and *out = 0 for zero.  The same
 * division-step inversion the device pre-pass runs; pg_scalar_invert_fermat is a^(q-2), its independent cross-check. */
pg_status pg_scalar_invert(const pg_scalar *a, pg_scalar *out);
pg_status pg_scalar_invert_fermat(const pg_scalar *a, pg_scalar *out);
uint64_t pg_bits_count(const pg_scalar *s);                    /* src/range.rs:173-181 */
uint64_t pg_num_bits_closest_power_of_two(const pg_scalar *s); /* src/range.rs:185-189 */

/* ---- the data format on the way in and out -------------------------------------------
 * A BlsScalar travels as 32 little-endian bytes of its canonical value (dusk-bytes Serializable, what
 * src/range.rs:162 reads back with to_bytes); the kernels want Montgomery limbs.  Both conversions in bulk, device to
 * device, 16-byte aligned buffers of 32 * batch bytes:
 *   from_canonical  BlsScalar::from_bytes per element; an encoding >= q (from_bytes returns Err) becomes 0, is flagged in
 *                   d_bad_mask (may be NULL) and counted; PG_ERR_BAD_ENCODING if any -- the output is complete all the
 *                   same -- while PG_ERR_INVALID_ARGUMENT keeps meaning a bad pointer (synchronises `stream`).  It counts
 *                   in the engine's scratch, the plan calls' error count: like them it is ordered behind the engine's
 *                   previous call on another stream, and the next one behind it.  The count comes back in a word of its
 *                   own: what pg_plan_result reports of an earlier plan is left alone
 *   to_canonical    BlsScalar::to_bytes per element; uses no engine scratch and takes no part in that ordering */
pg_status pg_scalars_from_canonical_batch(pg_engine *e, const void *d_bytes, uint64_t batch, pg_scalar *d_out,
                                          uint8_t *d_bad_mask, uint64_t *bad_count /* may be NULL */, void *stream);
pg_status pg_scalars_to_canonical_batch(pg_engine *e, const pg_scalar *d_scalars, uint64_t batch, void *d_bytes, void *stream);

/* ---- range gadgets, batched --------------------------------------------
 * pg_range_check_batch: for every witness i, in order,
 *     w = AllocatedScalar::allocate(composer, witness[i]);   src/allocated_scalar.rs:27
 *     result[i] = range_check(composer, min, max, w);        src/range.rs:27-43
 * emitting 4n+11 rows and 2n+524 variables per witness, rows and variables
 * numbered exactly as that loop numbers them starting at (gate_base,
 * var_base).  n = num_bits_closest_power_of_two(max - 1). */
pg_status pg_range_check_layout(const pg_scalar *min_range, const pg_scalar *max_range, uint64_t batch,
                                pg_layout *out);
pg_status pg_range_check_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range,
                               const pg_scalar *d_witness, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                               const pg_columns *out, pg_variable *d_result_vars /* may be NULL */, void *stream);

/* The rows of pg_range_check_batch WITHOUT the witnesses: selectors and wire indices are a function of the public
 * bounds and of the numbering alone, so a process that is sent only another process's variable table (32 B per
 * variable instead of 184 B per row on top) regenerates the rest locally.  out->var_values is not written and may be
 * NULL.  The result Variable of item i is var_base + (i + 1) * vars_per_item - 1. */
pg_status pg_range_check_structure_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range, uint64_t batch,
                                         uint64_t gate_base, uint64_t var_base, const pg_columns *out, void *stream);

/* ---- witness refresh: the variable assignments of a batched call, and nothing else ---------------------------------
 * The reference's prover flow builds a circuit once, preprocesses it, and then rebuilds the SAME circuit with other witnesses
 * (prover.clear_witness(); gadget calls again; prove -- tests/scalar_gadgets_tests.rs:108-119, 168-177): selectors, wire
 * indices and numbering are a function of the public inputs (the verifier builds them from other witnesses altogether, :36 vs
 * :43), only the assignments change.  A *_values_batch call writes exactly what the full call writes into out->var_values --
 * d_var_values[k] = the assignment of the call's k-th variable, limb for limb -- and touches no row: 32 B per variable instead
 * of 184 B per row on top (33 of the 223 KB a 256-bit range_check item weighs).  Numbering does not enter (no gate_base /
 * var_base: an assignment does not depend on its Variable's index). */
pg_status pg_range_check_values_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range,
                                      const pg_scalar *d_witness, uint64_t batch, pg_scalar *d_var_values, void *stream);
pg_status pg_max_bound_values_batch(pg_engine *e, const pg_scalar *max_range, const pg_scalar *d_witness, uint64_t batch,
                                    pg_scalar *d_var_values, void *stream);
/* ragged: the plan of the bounds (pg_max_bound_ragged_plan) is public structure and is reused as it is */
pg_status pg_max_bound_ragged_values_batch(pg_engine *e, const pg_scalar *d_max_range, const pg_scalar *d_witness, uint64_t batch,
                                           const uint32_t *d_num_bits, const uint64_t *d_row_off, const uint64_t *d_var_off,
                                           pg_scalar *d_var_values, void *stream);
/* the fused mix: an item's SHAPE depends on its witness (is_non_zero stops at v = 0, src/scalar.rs:79), so the refresh plans
 * again -- d_row_off / d_var_off / d_err_mask (may be NULL) are OUTPUTS as in pg_scalar_mix_planned_batch, the totals come
 * from pg_plan_result -- and the caller compares them with the circuit it preprocessed: other totals or another error mask
 * mean another circuit. */
pg_status pg_scalar_mix_values_batch(pg_engine *e, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                                     const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, uint64_t *d_row_off,
                                     uint64_t *d_var_off, uint8_t *d_err_mask /* may be NULL */, pg_scalar *d_var_values,
                                     void *stream);

/* pg_range_check_allocated_batch: the gadget alone, on witnesses that are ALREADY allocated --
 *     result[i] = range_check(composer, min, max, AllocatedScalar { var: d_witness_var[i], scalar: d_witness[i] });
 * 4n+11 rows and 2n+523 variables per item (no allocate). */
pg_status pg_range_check_allocated_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range,
                                         const pg_variable *d_witness_var, const pg_scalar *d_witness, uint64_t batch,
                                         uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                         pg_variable *d_result_vars /* may be NULL */, void *stream);

/* scalar_decomposition_gadget(composer, num_bits, witness) -> (is_equal, bit Variables)   src/range.rs:119-158
 * (private in the reference, exercised by its unit test at :205-233): per item 2*num_bits+4 rows and num_bits+260
 * variables; the bit Variables of item i are var_base + i*(num_bits+260) + [0, num_bits), is_equal is the item's
 * last variable.  num_bits > 256 -> PG_ERR_INVALID_ARGUMENT (the reference panics on the slice, :134). */
pg_status pg_scalar_decomposition_layout(uint64_t num_bits, uint64_t batch, pg_layout *out);
pg_status pg_scalar_decomposition_batch(pg_engine *e, uint64_t num_bits, const pg_variable *d_witness_var,
                                        const pg_scalar *d_witness, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                        const pg_columns *out, pg_variable *d_result_vars /* may be NULL */, void *stream);

/* pg_max_bound_batch: one public bound for the whole batch.  For every witness i,
 *     w = AllocatedScalar::allocate(composer, witness[i]);
 *     (result[i], n) = max_bound(composer, max_range, w);             src/range.rs:82-113
 * 2n+5 rows and n+262 variables per witness; layout->num_bits is the u64 the reference returns. */
pg_status pg_max_bound_layout(const pg_scalar *max_range, uint64_t batch, pg_layout *out);
pg_status pg_max_bound_batch(pg_engine *e, const pg_scalar *max_range, const pg_scalar *d_witness, uint64_t batch,
                             uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                             pg_variable *d_result_vars /* may be NULL */, void *stream);

/* same, on already-allocated witnesses: 2n+5 rows and n+261 variables per item */
pg_status pg_max_bound_allocated_batch(pg_engine *e, const pg_scalar *max_range, const pg_variable *d_witness_var,
                                       const pg_scalar *d_witness, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                       const pg_columns *out, pg_variable *d_result_vars /* may be NULL */, void *stream);

/* Ragged max_bound: one public bound PER ITEM (device array), so the ladder length n_i and with it the rows
 * (2 n_i + 5) and variables (n_i + 262) of an item depend on public data.  The plan computes n_i
 * (src/range.rs:87-90) and the exclusive prefix sums of rows / variables on the device, returns the totals
 * (it synchronises `stream`), and the batch call emits at those offsets.
 * Caller-allocated device buffers: d_num_bits[batch] (u32), d_row_off[batch+1], d_var_off[batch+1] (u64). */
pg_status pg_max_bound_ragged_plan(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                   uint64_t *d_row_off, uint64_t *d_var_off, pg_layout *out, void *stream);
pg_status pg_max_bound_ragged_batch(pg_engine *e, const pg_scalar *d_max_range, const pg_scalar *d_witness,
                                    uint64_t batch, const uint32_t *d_num_bits, const uint64_t *d_row_off,
                                    const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base,
                                    const pg_columns *out, pg_variable *d_result_vars /* may be NULL */, void *stream);

/* Ragged range_check: one public (min, max) pair PER ITEM (two device arrays).  For every item i,
 *     w = AllocatedScalar::allocate(composer, witness[i]);
 *     result[i] = range_check(composer, min[i], max[i], w);               src/range.rs:27-43
 * The ladder length n_i comes from max[i] alone (min_bound reuses it, :34-37): 4 n_i + 11 rows and 2 n_i + 524 variables per
 * item, at most 1031 and 1034.  The plan is pg_max_bound_ragged_plan's with these weights (same buffers, same totals, it
 * synchronises `stream`); the batch call emits at its offsets, the values call writes the assignments alone (a witness refresh
 * under the plan of the same bounds). */
pg_status pg_range_check_ragged_plan(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                     uint64_t *d_row_off, uint64_t *d_var_off, pg_layout *out, void *stream);
pg_status pg_range_check_ragged_batch(pg_engine *e, const pg_scalar *d_min_range, const pg_scalar *d_max_range,
                                      const pg_scalar *d_witness, uint64_t batch, const uint32_t *d_num_bits,
                                      const uint64_t *d_row_off, const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base,
                                      const pg_columns *out, pg_variable *d_result_vars /* may be NULL */, void *stream);
pg_status pg_range_check_ragged_values_batch(pg_engine *e, const pg_scalar *d_min_range, const pg_scalar *d_max_range,
                                             const pg_scalar *d_witness, uint64_t batch, const uint32_t *d_num_bits,
                                             const uint64_t *d_row_off, const uint64_t *d_var_off, pg_scalar *d_var_values,
                                             void *stream);

/* Asynchronous plans: enqueue and return at once; the totals (and the error count) land in engine-owned pinned host
 * memory and are read with pg_plan_result once the stream has been synchronised.  For callers that pre-allocate
 * worst-case buffers (10 rows / 15 variables per mix item, 515 rows / 517 variables per max_bound item, 1031 / 1034 per range_check item) and do not
 * want a host round trip between the plan and the emit call. */
pg_status pg_max_bound_ragged_plan_async(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                         uint64_t *d_row_off, uint64_t *d_var_off, void *stream);
pg_status pg_range_check_ragged_plan_async(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                           uint64_t *d_row_off, uint64_t *d_var_off, void *stream);
pg_status pg_scalar_mix_plan_async(pg_engine *e, const pg_scalar *d_v, uint64_t batch, uint64_t *d_row_off,
                                   uint64_t *d_var_off, uint8_t *d_err_mask /* may be NULL */, void *stream);
/* totals of the engine's most recent plan; PG_ERR_NON_EXISTING_INVERSE when that plan found failing items */
pg_status pg_plan_result(pg_engine *e, pg_layout *out, uint64_t *err_count /* may be NULL */);

/* ---- scalar gadgets, batched ----------------------------------------------
 * The stand-alone gadgets take EXISTING Variables: d_*_var are their indices, d_*_val their assignments (what
 * the reference reads from composer.variables).  Each emits, per item i and in order, the rows/variables of
 *   conditionally_select_zero(composer, x, select) -> Variable          src/scalar.rs:21-27   (1 row, 1 var)
 *   conditionally_select_one(composer, y, selector) -> Variable         src/scalar.rs:36-59   (4 rows, 4 vars)
 *   maybe_equal(composer, a, b) -> Variable                             src/scalar.rs:105-140 (3 rows, 3 vars)
 *   is_non_zero(composer, var, value_assigned) -> Result<(), Error>     src/scalar.rs:63-97   (3 rows, 3 vars) */
pg_status pg_conditionally_select_zero_batch(pg_engine *e, const pg_variable *d_x_var, const pg_scalar *d_x_val,
                                             const pg_variable *d_select_var, const pg_scalar *d_select_val,
                                             uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                             const pg_columns *out, pg_variable *d_result_vars, void *stream);
pg_status pg_conditionally_select_one_batch(pg_engine *e, const pg_variable *d_y_var, const pg_scalar *d_y_val,
                                            const pg_variable *d_selector_var, const pg_scalar *d_selector_val,
                                            uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                            const pg_columns *out, pg_variable *d_result_vars, void *stream);
pg_status pg_maybe_equal_batch(pg_engine *e, const pg_variable *d_a_var, const pg_scalar *d_a_val,
                               const pg_variable *d_b_var, const pg_scalar *d_b_val, uint64_t batch,
                               uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                               pg_variable *d_result_vars, void *stream);
/* is_non_zero returns Err(NonExistingInverse) AFTER one variable and one row were pushed (src/scalar.rs:69-79):
 * an item whose value is 0 therefore occupies 1 row / 1 variable instead of 3 / 3 and the batch is ragged.
 * The plan writes the per-item error mask (1 = Err), the prefix sums and the totals; it returns
 * PG_ERR_NON_EXISTING_INVERSE when any item failed (the layout is still valid and the batch may be emitted:
 * it reproduces a loop that records the error and carries on) and synchronises `stream`. */
pg_status pg_is_non_zero_plan(pg_engine *e, const pg_scalar *d_value_assigned, uint64_t batch, uint64_t *d_row_off,
                              uint64_t *d_var_off, uint8_t *d_err_mask /* may be NULL */, pg_layout *out,
                              uint64_t *err_count /* may be NULL */, void *stream);
pg_status pg_is_non_zero_batch(pg_engine *e, const pg_variable *d_var, const pg_scalar *d_value_assigned,
                               uint64_t batch, const uint64_t *d_row_off, const uint64_t *d_var_off,
                               uint64_t gate_base, uint64_t var_base, pg_variable zero_var, const pg_columns *out,
                               void *stream);

/* The fused mix (BASELINE.json config 3), one launch: per item
 *     v, y, s = composer.add_input x3; a, b = AllocatedScalar::allocate x2;
 *     is_non_zero(composer, v_var, v); conditionally_select_one(composer, y_var, s_var); maybe_equal(composer, a, b)
 * 10 rows + 15 variables per item (8 + 13 where v = 0).  d_result_vars[2i] = select_one's Variable,
 * d_result_vars[2i+1] = maybe_equal's.  Plan semantics as pg_is_non_zero_plan. */
pg_status pg_scalar_mix_plan(pg_engine *e, const pg_scalar *d_v, uint64_t batch, uint64_t *d_row_off,
                             uint64_t *d_var_off, uint8_t *d_err_mask /* may be NULL */, pg_layout *out,
                             uint64_t *err_count /* may be NULL */, void *stream);
pg_status pg_scalar_mix_batch(pg_engine *e, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                              const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, const uint64_t *d_row_off,
                              const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base, pg_variable zero_var,
                              const pg_columns *out, pg_variable *d_result_vars /* may be NULL */, void *stream);
/* Plan and emit in ONE call, for callers whose buffers hold the worst case (`out`: 10 rows and 15 variables per item;
 * d_row_off / d_var_off: batch + 1 entries, written by the call).  Same result as pg_scalar_mix_plan_async followed by
 * pg_scalar_mix_batch on the same stream; the totals and the error count are read with pg_plan_result after the stream has
 * been synchronised.  What the single call buys: no plan launch at all -- the launch that inverts reads every v anyway and
 * makes the prefix sums on its way (~7 % of a 2^20-item step). */
pg_status pg_scalar_mix_planned_batch(pg_engine *e, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                                      const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, uint64_t *d_row_off,
                                      uint64_t *d_var_off, uint8_t *d_err_mask /* may be NULL */, uint64_t gate_base,
                                      uint64_t var_base, pg_variable zero_var, const pg_columns *out,
                                      pg_variable *d_result_vars /* may be NULL */, void *stream);

/* ---- pg_composer: the composer-gate API surface, device resident ----------------------------
 * The counterpart of the slice of dusk-plonk's `StandardComposer` the reference's gadgets call.  Columns and the
 * variable table live in HBM with fixed capacities chosen at creation (PG_ERR_CAPACITY when an append does not fit);
 * every call appends on the composer's stream and returns immediately -- Variables are numbered on the host, their
 * values exist only on the device.  With the single-gadget entry points below (the reference's exact signatures,
 * argument order and error behaviour) host code written against the reference reads the same:
 *
 *     reference (tests/range_gadgets_tests.rs:36-43)                 this library
 *     let w = AllocatedScalar::allocate(composer, witness);          pg_allocated_scalar_allocate(c, &witness, &w);
 *     let r = range_check(composer, min, max, w);                    pg_range_check(c, &min, &max, &w, &r);
 *     composer.constrain_to_constant(r, outcome, None);              pg_composer_constrain_to_constant(c, r, &outcome, NULL);
 */
typedef struct pg_composer pg_composer;

/* StandardComposer::new() [with_dummy = 1]: zero_var = Variable(0) + its constant row, then the two dummy
 * constraints (variables 1..4 = 6, 1, 7, -20): 3 rows, 5 variables.  with_dummy = 0 stops after zero_var. */
pg_status pg_composer_create(pg_engine *e, uint64_t gate_capacity, uint64_t var_capacity, int with_dummy, void *stream,
                             pg_composer **out);
void pg_composer_destroy(pg_composer *c);
uint64_t pg_composer_circuit_size(const pg_composer *c);  /* StandardComposer::circuit_size(): rows so far */
uint64_t pg_composer_num_variables(const pg_composer *c);
pg_variable pg_composer_zero_var(const pg_composer *c);
/* device pointers to the live columns (row 0 = gate 0, var_values[0] = Variable(0)); they move when the composer grows */
pg_status pg_composer_columns(const pg_composer *c, pg_columns *out);
/* Capacity.  The reference's composer is a set of Vecs that grow on their own; here growth is an explicit decision
 * because it re-allocates HBM and copies the live part (device to device, on the composer's stream):
 *   pg_composer_reserve    make room for at least that many rows / Variables in total (never shrinks);
 *   pg_composer_auto_grow  on = an append that does not fit doubles the capacity it ran out of (at least to what the
 *                          append needs) instead of returning PG_ERR_CAPACITY; off (the default) = fixed capacity. */
pg_status pg_composer_reserve(pg_composer *c, uint64_t gate_capacity, uint64_t var_capacity);
pg_status pg_composer_auto_grow(pg_composer *c, int on);
/* Where the composer's columns lie (see pg_columns_slab_layout below): stride_bytes > 0 moves the nine arrays into ONE
 * allocation with the selector columns that far apart (live rows and variables are copied; later growth keeps the layout and
 * needs room for the old block and the new one at once); 0 goes back to nine separate allocations.  For a composer of a few
 * GB on a card with room to spare: 24 GiB.  The columns move: pointers from pg_composer_columns are stale afterwards. */
pg_status pg_composer_spread_columns(pg_composer *c, uint64_t stride_bytes);
uint64_t pg_composer_gate_capacity(const pg_composer *c);
uint64_t pg_composer_var_capacity(const pg_composer *c);
pg_status pg_composer_sync(pg_composer *c);
/* The command queue.  The reference's usage is ONE composer call at a time (tests/range_gadgets_tests.rs:29-44:
 * allocate, range_check, constrain_to_constant, ...); a launch per call would make that loop launch-bound.  Variables
 * are numbered on the host and their assignments live on the device, so the single calls -- the gate calls below,
 * pg_allocated_scalar_allocate, pg_range_check, pg_max_bound, and the four scalar gadgets (which are sequences of those
 * gate calls, src/scalar.rs, and are composed of them here) -- are RECORDED (arguments checked, numbering advanced,
 * results returned at once) and reach the composer's stream, in order, when anything needs them: pg_composer_sync /
 * _columns / _copy_out / _read_value / _check / _dense_pi / _materialize / _permutation, any batched append,
 * pg_scalar_decomposition_gadget, a capacity change, a full queue (8192 entries), or pg_composer_flush.  A run of gate calls is ONE launch
 * (the outputs of add / mul computed in command order, level by level); a run of `allocate + range_check` (or
 * max_bound) pairs with the same public bounds -- the reference's loop -- is ONE batched emit launch, and leaves the
 * batched append's footprint for pg_composer_materialize / _permutation (runs of >= 4096 rows).  The loop as the
 * reference's tests write it -- the pair, then up to eight gate calls that create no Variable (constrain_to_constant on
 * the result, assert_equal, ...), per witness -- is ONE emit launch too (its items that many rows apart) plus one run of
 * gates: a row's place is assigned when its call is recorded, and a rows-only gate reads no assignment.  Where those
 * gates constrain the gadget's own result (its Variable on all three wires) the loop leaves a footprint as well.
 *   pg_composer_queue(c, 0) flushes and turns recording off (one launch per call, as before); on by default. */
pg_status pg_composer_queue(pg_composer *c, int on);
pg_status pg_composer_flush(pg_composer *c);
/* entries waiting, flushes so far, launches those flushes took (any pointer may be NULL) */
pg_status pg_composer_queue_stats(const pg_composer *c, uint64_t *pending, uint64_t *flushes, uint64_t *launches);

/* Witness refresh.  The reference's tests prove twice with one preprocessed circuit: prover.clear_witness(), the same
 * gadget calls on other witnesses, prove again (tests/scalar_gadgets_tests.rs:108-119, 168-177, 226-235; dusk-plonk's
 * Prover::clear_witness() = a fresh StandardComposer).  pg_composer_clear_witness does the same -- rows and Variables
 * count from StandardComposer::new()'s state again, public inputs are forgotten -- but the device columns stay where
 * they are: an append that repeats, at the same place in the call sequence, what the build before it did there (the same
 * call with the same public parameters, landing on the same first row, first Variable and zero_var) finds its rows in the
 * columns and writes only its assignments (32 B per variable instead of 184 B per row on top; pg_*_values_batch).  That
 * holds for every append: single composer gate calls and single gadget calls, the batched appends on witness scalars, and the
 * batched appends whose rows depend on device arrays (Variables, per-item bounds), which are signed by a 128-bit digest of
 * those arrays taken in the pass that validates them.  The two gadgets whose SHAPE depends on witness values --
 * is_non_zero and the fused mix, which stop at a zero (src/scalar.rs:79) -- are found in place only when no item fails, in
 * either build.  The first append that differs from the previous build ends the refresh: from there on everything is emitted
 * in full, so another circuit is built correctly too -- only slower. */
pg_status pg_composer_clear_witness(pg_composer *c);
/* since the last pg_composer_clear_witness: rows found in place, rows written again, still matching (any pointer may be NULL) */
pg_status pg_composer_refresh_stats(const pg_composer *c, uint64_t *rows_in_place, uint64_t *rows_rewritten, int *refreshing);

/* composer calls used by the gadgets (same argument order as dusk-plonk 0.8; `pi` may be NULL = None) */
pg_status pg_composer_add_input(pg_composer *c, const pg_scalar *s, pg_variable *out);
pg_status pg_composer_add_witness_to_circuit_description(pg_composer *c, const pg_scalar *value, pg_variable *out);
pg_status pg_composer_constrain_to_constant(pg_composer *c, pg_variable a, const pg_scalar *constant, const pg_scalar *pi);
pg_status pg_composer_assert_equal(pg_composer *c, pg_variable a, pg_variable b);
pg_status pg_composer_poly_gate(pg_composer *c, pg_variable a, pg_variable b, pg_variable o, const pg_scalar *q_m,
                                const pg_scalar *q_l, const pg_scalar *q_r, const pg_scalar *q_o, const pg_scalar *q_c,
                                const pg_scalar *pi);
pg_status pg_composer_add(pg_composer *c, const pg_scalar *q_l, pg_variable a, const pg_scalar *q_r, pg_variable b,
                          const pg_scalar *q_c, const pg_scalar *pi, pg_variable *out);
pg_status pg_composer_mul(pg_composer *c, const pg_scalar *q_m, pg_variable a, pg_variable b, const pg_scalar *q_c,
                          const pg_scalar *pi, pg_variable *out);
pg_status pg_composer_mul_gate(pg_composer *c, pg_variable a, pg_variable b, pg_variable o, const pg_scalar *q_m,
                               const pg_scalar *q_o, const pg_scalar *q_c, const pg_scalar *pi);
pg_status pg_composer_boolean_gate(pg_composer *c, pg_variable a);

/* the reference's public API, one call = one gadget (src/lib.rs:42-45) */
pg_status pg_allocated_scalar_allocate(pg_composer *c, const pg_scalar *scalar, pg_allocated_scalar *out); /* src/allocated_scalar.rs:27 */
pg_status pg_range_check(pg_composer *c, const pg_scalar *min_range, const pg_scalar *max_range,
                         const pg_allocated_scalar *witness, pg_variable *out);                           /* src/range.rs:27-43 */
pg_status pg_max_bound(pg_composer *c, const pg_scalar *max_range, const pg_allocated_scalar *witness, pg_variable *out,
                       uint64_t *num_bits);                                                               /* src/range.rs:82-113 */
/* src/range.rs:119-123; d_bits_out (host, may be NULL) receives the first num_bits bit Variables */
pg_status pg_scalar_decomposition_gadget(pg_composer *c, uint64_t num_bits, const pg_allocated_scalar *witness,
                                         pg_variable *is_equal, pg_variable *bits_out);
pg_status pg_conditionally_select_zero(pg_composer *c, pg_variable x, pg_variable select, pg_variable *out); /* src/scalar.rs:21-27 */
pg_status pg_conditionally_select_one(pg_composer *c, pg_variable y, pg_variable selector, pg_variable *out); /* src/scalar.rs:36-59 */
/* PG_ERR_NON_EXISTING_INVERSE after the first variable + row were appended, like the reference (src/scalar.rs:69-79) */
pg_status pg_is_non_zero(pg_composer *c, pg_variable var, const pg_scalar *value_assigned);              /* src/scalar.rs:63-97 */
pg_status pg_maybe_equal(pg_composer *c, const pg_allocated_scalar *a, const pg_allocated_scalar *b, pg_variable *out); /* src/scalar.rs:105-140 */

/* batched appends: the loop  for w in d_witness { allocate; range_check }  emitted at the composer's end */
pg_status pg_composer_range_check_batch(pg_composer *c, const pg_scalar *min_range, const pg_scalar *max_range,
                                        const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars);

/* AllocatedScalar::allocate of a batch (src/allocated_scalar.rs:27): the loop  for s in d_scalars { add_input(s) };
 * the Variables are *first_var, *first_var + 1, ...  (d_scalars: device, reduced) */
pg_status pg_composer_add_input_batch(pg_composer *c, const pg_scalar *d_scalars, uint64_t batch, pg_variable *first_var);
/* the loop  for i { range_check(composer, min, max, AllocatedScalar { var: d_witness_var[i], scalar: d_witness[i] }) }
 * on witnesses allocated before (device arrays; every d_witness_var[i] must be a Variable of this composer -- the
 * reference panics on an unknown one; here EVERY batched append that takes Variables checks its arrays on the device
 * first (one small reduction and one host synchronisation) and returns PG_ERR_INVALID_ARGUMENT with nothing appended) */
pg_status pg_composer_range_check_allocated_batch(pg_composer *c, const pg_scalar *min_range, const pg_scalar *max_range,
                                                  const pg_variable *d_witness_var, const pg_scalar *d_witness,
                                                  uint64_t batch, pg_variable *d_result_vars);

/* the other uniform gadgets as batched appends, each the loop over i of the reference call named:
 *   max_bound:            allocate(d_witness[i]); max_bound(composer, max_range, w)        src/range.rs:82-113
 *   max_bound_allocated:  max_bound(composer, max_range, AllocatedScalar { d_witness_var[i], d_witness[i] })
 *   scalar_decomposition: scalar_decomposition_gadget(composer, num_bits, AllocatedScalar { .. })   src/range.rs:119-158
 *                         (bit Variables of item i: first new Variable + i * (num_bits + 260) + [0, num_bits))
 *   conditionally_select_zero / _one, maybe_equal: on EXISTING Variables (device index arrays); their assignments
 *                         are read from the composer's own variable table, as the reference reads composer.variables
 * *num_bits (may be NULL) is the u64 max_bound returns. */
pg_status pg_composer_max_bound_batch(pg_composer *c, const pg_scalar *max_range, const pg_scalar *d_witness, uint64_t batch,
                                      pg_variable *d_result_vars, uint64_t *num_bits);
pg_status pg_composer_max_bound_allocated_batch(pg_composer *c, const pg_scalar *max_range, const pg_variable *d_witness_var,
                                                const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars,
                                                uint64_t *num_bits);
pg_status pg_composer_scalar_decomposition_batch(pg_composer *c, uint64_t num_bits, const pg_variable *d_witness_var,
                                                 const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars);
pg_status pg_composer_conditionally_select_zero_batch(pg_composer *c, const pg_variable *d_x_var,
                                                      const pg_variable *d_select_var, uint64_t batch,
                                                      pg_variable *d_result_vars);
pg_status pg_composer_conditionally_select_one_batch(pg_composer *c, const pg_variable *d_y_var,
                                                     const pg_variable *d_selector_var, uint64_t batch,
                                                     pg_variable *d_result_vars);
pg_status pg_composer_maybe_equal_batch(pg_composer *c, const pg_variable *d_a_var, const pg_variable *d_b_var, uint64_t batch,
                                        pg_variable *d_result_vars);

/* range_gate(witness, num_bits): witness < 2^num_bits by a quad-accumulator widget on the composer's three wires (what the
 * reference's src/range.rs:11 points its users to for a power-of-two bound; not dusk-plonk's four-wire widget: DESIGN 3.19).
 * num_bits even, 2 <= num_bits <= 254, else PG_ERR_INVALID_ARGUMENT with nothing appended.  With k = num_bits / 2,
 * g = ceil(k / 3), pad = 3g - k and v the witness's canonical integer, positions p = 0 .. 3g hold
 *   P(p) = zero_var (p <= pad);  a new Variable first + (p - pad - 1) of value v >> 2 (3g - p) (pad < p < 3g);  P(3g) = witness
 * and the item owns g + 1 rows and k - 1 new Variables: row i < g = (P(3i), P(3i+1), P(3i+2)) with q_range = 1, row g =
 * (witness, zero_var, zero_var) with q_range = 0, all five arithmetic selectors 0.  A row with q_range = 1 states that each
 * of b - 4a, c - 4b and a_next - 4c lies in {0, 1, 2, 3}.  An out-of-range witness still gets all its rows (its row 0 fails).
 * On EXISTING Variables, their assignments read from the composer's own table; the batched form checks its array on the
 * device first.  q_range is written by pg_composer_materialize; pg_composer_check also checks these rows' statements. */
pg_status pg_composer_range_gate(pg_composer *c, pg_variable witness, uint64_t num_bits);
pg_status pg_composer_range_gate_batch(pg_composer *c, const pg_variable *d_witness_var, uint64_t num_bits, uint64_t batch);

/* interval_gate(witness, min, max, num_bits): min <= witness <= max for PUBLIC bounds, by two range widgets (above) on the
 * differences d = witness - min (half h = 0) and d = max - witness (h = 1); DESIGN 3.20.  Preconditions, else
 * PG_ERR_INVALID_ARGUMENT with nothing appended: num_bits even, 2 <= num_bits <= 252 (2^(num_bits + 1) < r: the two differences
 * cannot add up across the modulus), and, as canonical integers, min <= max and max - min < 2^num_bits.  With k, g and pad as for
 * range_gate an item owns 2 (g + 1) rows and 2 k new Variables; half h takes rows h (g + 1) .. and Variables first + h k ..:
 *   first + h k + kk = c(d) >> 2 (k - 1 - kk), kk = 0 .. k - 1 (c(d) the canonical integer of d: k - 1 accumulators, then d itself)
 *   P(p) = zero_var (p <= pad);  first + h k + (p - pad - 1) (pad < p <= 3g, so P(3g) = d)
 *   row i < g = (P(3i), P(3i+1), P(3i+2)), q_range = 1, all five arithmetic selectors 0
 *   row g = (d, witness, zero_var), q_range = 0, q_l = 1 and  q_r = -1, q_c = +min (h = 0: d - w + min = 0)
 *                                                             q_r = +1, q_c = -max (h = 1: d + w - max = 0)
 * The widget rows are, row for row, those of 2 range_gate items: q_range is written by pg_composer_materialize and their
 * statements checked by pg_composer_check as for range_gate; the terminal rows are ordinary arithmetic rows.  A witness outside
 * [min, max] still gets all its rows: row 0 of the half whose difference is negative fails.
 * On EXISTING Variables, their assignments read from the composer's own table.  _batch: one host pair (min, max) for the call.
 * _ragged_batch: device arrays with a pair per item (Montgomery form, like every pg_scalar), validated on the device before
 * anything is appended; the error message names the first item whose pair violates a precondition. */
pg_status pg_composer_interval_gate(pg_composer *c, pg_variable witness, const pg_scalar *min, const pg_scalar *max, uint64_t num_bits);
pg_status pg_composer_interval_gate_batch(pg_composer *c, const pg_variable *d_witness_var, const pg_scalar *min, const pg_scalar *max,
                                          uint64_t num_bits, uint64_t batch);
pg_status pg_composer_interval_gate_ragged_batch(pg_composer *c, const pg_variable *d_witness_var, const pg_scalar *d_min,
                                                 const pg_scalar *d_max, uint64_t num_bits, uint64_t batch);

/* is_less_equal(x, y, num_bits, strict): the bit [x <= y] ([x < y] when strict != 0) of two WITNESSES as a Variable the rest of the
 * circuit can use, from ONE range widget (above) over num_bits + 2 bits on z = 2^num_bits + y - x - s, s = 1 if strict else 0;
 * DESIGN 3.23.  num_bits even, 2 <= num_bits <= 252 (2^(num_bits + 1) < r), else PG_ERR_INVALID_ARGUMENT with nothing appended and
 * the results untouched.  With K = num_bits + 2, k = K / 2, g = ceil(k / 3), pad = 3g - k and c(z) the canonical integer of z an item
 * owns g + 1 rows and k new Variables:
 *   first + kk = c(z) >> 2 (k - 1 - kk), kk = 0 .. k - 1: `first` is the top quad of c(z) -- the RESULT --, first + k - 1 is z
 *   P(p) = zero_var (p <= pad);  first + (p - pad - 1) (pad < p <= 3g, so P(3g) = z)
 *   row i < g = (P(3i), P(3i+1), P(3i+2)), q_range = 1, all five arithmetic selectors 0
 *   row g = (z, y, x), q_range = 0, q_l = 1, q_r = -1, q_o = +1, q_c = -2^num_bits + s   (z - y + x - 2^num_bits + s = 0)
 * PRECONDITION of the meaning, which the gadget does NOT enforce: the circuit bounds x and y below 2^num_bits (range_gate or
 * interval_gate at <= num_bits bits).  Then nothing wraps, the result is 0 or 1, and it is [x <= y] ([x < y] when strict).
 * Without it the rows state c(z) < 2^K alone and the result is a quad without meaning (x = r - 1, y = 0 gives 1).  An item whose
 * c(z) >= 2^K still gets all its rows; its row 0 fails.  On EXISTING Variables, their assignments read from the composer's own
 * table; the batched form checks its arrays on the device first.  d_result_vars[i] = (the call's first new Variable) + i k; it may
 * be NULL. */
pg_status pg_composer_is_less_equal(pg_composer *c, pg_variable x, pg_variable y, uint64_t num_bits, int strict, pg_variable *result);
pg_status pg_composer_is_less_equal_batch(pg_composer *c, const pg_variable *d_x_var, const pg_variable *d_y_var,
                                          uint64_t num_bits, int strict, uint64_t batch, pg_variable *d_result_vars);

/* the composer's gate calls over device arrays of Variables, one set of selectors for the whole batch (no public
 * inputs): the loops
 *   poly_gate:             for i { composer.poly_gate(a[i], b[i], c[i], q_m, q_l, q_r, q_o, q_c, None) }
 *   add / mul:             for i { out[i] = composer.add((q_l, a[i]), (q_r, b[i]), q_c, None) }  /  mul(q_m, a[i], b[i], q_c, None)
 *   constrain_to_constant: for i { composer.constrain_to_constant(a[i], constant, None) }
 *   boolean_gate:          for i { composer.boolean_gate(a[i]) }
 * every index must be a Variable of this composer (the reference panics on an unknown one; here the arrays are checked on
 * the device first: PG_ERR_INVALID_ARGUMENT, nothing appended). */
pg_status pg_composer_poly_gate_batch(pg_composer *c, const pg_variable *d_a, const pg_variable *d_b, const pg_variable *d_c,
                                      const pg_scalar *q_m, const pg_scalar *q_l, const pg_scalar *q_r, const pg_scalar *q_o,
                                      const pg_scalar *q_c, uint64_t batch);
pg_status pg_composer_add_batch(pg_composer *c, const pg_scalar *q_l, const pg_variable *d_a, const pg_scalar *q_r,
                                const pg_variable *d_b, const pg_scalar *q_c, uint64_t batch, pg_variable *d_out_vars);
pg_status pg_composer_mul_batch(pg_composer *c, const pg_scalar *q_m, const pg_variable *d_a, const pg_variable *d_b,
                                const pg_scalar *q_c, uint64_t batch, pg_variable *d_out_vars);
pg_status pg_composer_constrain_to_constant_batch(pg_composer *c, const pg_variable *d_a, const pg_scalar *constant, uint64_t batch);
pg_status pg_composer_boolean_gate_batch(pg_composer *c, const pg_variable *d_a, uint64_t batch);

/* weighted_sum_ragged_batch: result[s] = k[s] + sum over the terms t of segment s of c[t] * value(x[t]), the loop
 *   for s in segments:                  terms b = d_seg_off[s] .. e = d_seg_off[s + 1] - 1, m = e - b + 1 >= 2
 *       acc = composer.add((c[b], x[b]), (c[b+1], x[b+1]), k[s], None)
 *       for t in b+2 .. e: acc = composer.add((1, acc), (c[t], x[t]), 0, None)
 *       result[s] = acc
 * on EXISTING Variables x = d_term_var, their assignments read from the composer's own table.  With n0 rows and v0 Variables before
 * the call, term t with b < t <= e owns row n0 + (t - s - 1) and creates Variable v0 + (t - s - 1) (a segment's first term owns
 * neither): the call owns terms - segments rows and as many Variables, and result[s] = v0 + d_seg_off[s + 1] - s - 2.
 *   t = b+1:  wires (x[b], x[b+1], new)      q_m = 0  q_l = c[b]  q_r = c[b+1]  q_o = -1  q_c = k[s]
 *   t > b+1:  wires (new - 1, x[t], new)     q_m = 0  q_l = 1     q_r = c[t]    q_o = -1  q_c = 0
 * and the new Variable holds k[s] + sum_{i = b .. t} c[i] value(x[i]).  d_coeff [terms] or NULL: every coefficient 1; d_constant
 * [segments] or NULL: every constant 0 (Montgomery form, like every pg_scalar); d_result_vars [segments] or NULL.
 * Preconditions, else PG_ERR_INVALID_ARGUMENT with nothing appended: d_term_var and d_seg_off not NULL and 8-byte aligned, the
 * scalar arrays 16-byte aligned; terms < 2^32; every term a Variable of this composer; d_seg_off[0] == 0, d_seg_off[segments] ==
 * terms and every segment of at least 2 terms; every coefficient and constant reduced.  The arrays are validated on the device, in
 * one host synchronisation, before any entry of d_seg_off is used as an index; the message names the first offending segment,
 * coefficient or constant.  segments == 0 (terms must then be 0): PG_OK, nothing appended.
 * A one-term "sum" is x itself (or pg_composer_add_batch with a second operand): a caller who needs one in a ragged call pads the
 * segment with the composer's zero_var, which adds 0 whatever its coefficient.
 * The rows are ordinary arithmetic rows.  After pg_composer_clear_witness the same call -- same four arrays' contents, same place --
 * finds its rows and writes the assignments only. */
pg_status pg_composer_weighted_sum_ragged_batch(pg_composer *c, const pg_variable *d_term_var, const uint64_t *d_seg_off,
                                                const pg_scalar *d_coeff, const pg_scalar *d_constant, uint64_t terms, uint64_t segments,
                                                pg_variable *d_result_vars);
/* host only: the terms a workgroup takes per step (a power of two) and the tiles the carry launch scans at a time; a call of
 * more than tile_terms terms carries sums between tiles, one of more than tile_terms * tiles_per_carry_pass between passes */
pg_status pg_weighted_sum_geometry(uint32_t *tile_terms, uint32_t *tiles_per_carry_pass);

/* ragged batched appends: the composer plans the call itself (one host synchronisation for the totals), keeps the
 * per-item offsets for the permutation, and emits.
 *   max_bound_ragged: for i { allocate(d_witness[i]); max_bound(composer, d_max_range[i], w) } -- one public bound per
 *                     item; d_num_bits_out (device u32[batch], may be NULL) receives the u64 each call returns
 *   range_check_ragged: for i { allocate(d_witness[i]); range_check(composer, d_min_range[i], d_max_range[i], w) } -- one
 *                     public interval per item; d_num_bits_out as above.  After pg_composer_clear_witness the same call with
 *                     the same two bound arrays is found in place and only its assignments are written
 *   is_non_zero:      for i { is_non_zero(composer, d_var[i], value of d_var[i]) }; an item whose value is 0 stops after
 *                     its first variable + row (src/scalar.rs:69-79); returns PG_ERR_NON_EXISTING_INVERSE when any did
 *                     (everything is appended all the same, like a loop that records the error and carries on);
 *                     d_err_mask (device u8[batch]) and err_count may be NULL
 *   scalar_mix:       the fused item of pg_scalar_mix_batch (BASELINE config 3) */
pg_status pg_composer_max_bound_ragged_batch(pg_composer *c, const pg_scalar *d_max_range, const pg_scalar *d_witness,
                                             uint64_t batch, pg_variable *d_result_vars, uint32_t *d_num_bits_out);
pg_status pg_composer_range_check_ragged_batch(pg_composer *c, const pg_scalar *d_min_range, const pg_scalar *d_max_range,
                                               const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars,
                                               uint32_t *d_num_bits_out);
pg_status pg_composer_is_non_zero_batch(pg_composer *c, const pg_variable *d_var, uint64_t batch, uint8_t *d_err_mask,
                                        uint64_t *err_count);
pg_status pg_composer_scalar_mix_batch(pg_composer *c, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                                       const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch,
                                       pg_variable *d_result_vars, uint8_t *d_err_mask, uint64_t *err_count);

/* copy rows [gate_first, gate_first + n_gates) of the live columns and variables [var_first, var_first + n_vars)
 * into caller-owned device buffers (any member of dst may be NULL); enqueued on the composer's stream */
pg_status pg_composer_copy_out(pg_composer *c, uint64_t gate_first, uint64_t n_gates, uint64_t var_first, uint64_t n_vars,
                               const pg_columns *dst);

/* read-back and checks */
pg_status pg_composer_read_value(pg_composer *c, pg_variable v, pg_scalar *out); /* synchronises */
/* every row satisfies q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c + PI = 0?  *first_bad = -1 or the first failing row */
pg_status pg_composer_check(pg_composer *c, int64_t *first_bad);
/* construct_dense_pi_vec (tests/scalar_gadgets_tests.rs:151): d_out[circuit_size] */
pg_status pg_composer_dense_pi(pg_composer *c, pg_scalar *d_out);

/* everything else a prover-ready row holds.  Constant selector columns (q_4, q_arith = 1,
 * q_range = q_logic = q_fixed_group_add = q_variable_group_add = 0), w_4 (zero_var except on the dummy rows) and
 * the wire VALUE columns (variables[w_x[i]]).  Any pointer may be NULL (skipped); all are device arrays of
 * circuit_size entries. */
typedef struct pg_full_columns {
    pg_scalar *q_4, *q_arith, *q_range, *q_logic, *q_fixed_group_add, *q_variable_group_add;
    uint64_t *w_4;
    pg_scalar *w_l_value, *w_r_value, *w_o_value, *w_4_value;
} pg_full_columns;
pg_status pg_composer_materialize(pg_composer *c, const pg_full_columns *out);

/* the copy permutation the composer's bookkeeping implies (dusk-plonk's
 * Permutation::compute_sigma_permutations).  d_sigma[4 * padded_n] (device): sigma of position (wire, gate) at
 * index wire * padded_n + gate, encoded the same way; wire 0..3 = left, right, output, fourth; rows >= circuit_size
 * map to themselves.  padded_n >= circuit_size (the prover pads to a power of two).  Enqueued on the composer's
 * stream (one host synchronisation inside, to size the sorted list); scratch is kept by the composer and only grows. */
pg_status pg_composer_permutation(pg_composer *c, uint64_t padded_n, uint64_t *d_sigma);
/* Size of the sorted list of wire positions that refer to Variables created outside their own item (plus every position
 * of rows appended by single calls) for the NEXT pg_composer_permutation call; 0 = the composer's own estimate.  A
 * figure that is too small costs a second pass (the first reports the size needed), never a wrong result. */
pg_status pg_composer_permutation_reserve(pg_composer *c, uint64_t sparse_positions);

/* Satisfiability of the rows of ONE batch call whose wires all point into its own variables (the allocate-style
 * batches: range_check, max_bound, scalar_mix): q_m a b + q_l a + q_r b + q_o c + q_c = 0 on every row, with
 * a/b/c = var_values[wire - var_base] (a wire equal to zero_var reads as 0: is_non_zero's assert_equal row).
 * *first_bad = -1, or the first row that fails or references any other Variable outside
 * [var_base, var_base + n_vars).  Synchronises `stream`.  A size-independent property check: it scales to
 * the full 2^20-item batches where a limb-for-limb comparison with the CPU oracle does not. */
pg_status pg_check_rows(pg_engine *e, const pg_columns *cols, uint64_t n_gates, uint64_t var_base, uint64_t n_vars,
                        pg_variable zero_var, int64_t *first_bad, void *stream);

/* ---- the copy permutation as field elements: sigma evaluations and PLONK's grand product z ------------------------------
 * dusk-plonk 0.8's Permutation::compute_permutation_lagrange and compute_(fast_)permutation_poly, in evaluation form, over the
 * domain of padded_n = 2^m rows.  Engine-level calls over caller arrays (from pg_composer_materialize / _permutation or
 * anywhere else).  Conventions [DEP-RECALL] (the Python layer's defaults; arguments here):
 *   k = (1, K1, K2, K3) = (1, 7, 13, 17), one coset constant per wire, in sigma's wire order (left, right, output, fourth);
 *   omega = ROOT_OF_UNITY^(2^(32 - m)), ROOT_OF_UNITY = 7^t with q - 1 = 2^32 t (pg_domain_generator).
 * Host: the generator of the 2^log2_n subgroup (log2_n <= 32), Montgomery form. */
pg_status pg_domain_generator(uint32_t log2_n, pg_scalar *out);
/* d_out[4 * padded_n] = k[s / padded_n] * omega^(s mod padded_n) for s = d_sigma[p] (padded_n a power of two <= 2^32).  An
 * entry s >= 4 * padded_n -> PG_ERR_INVALID_ARGUMENT (found on the device; nothing is read out of bounds).  Synchronises. */
pg_status pg_sigma_evaluations(pg_engine *e, const uint64_t *d_sigma, uint64_t padded_n, const pg_scalar *omega, const pg_scalar k[4],
                               pg_scalar *d_out, void *stream);
/* The copy permutation's grand product: with num_i = prod_j (w_j[i] + beta k_j omega^i + gamma) and
 * den_i = prod_j (w_j[i] + beta sigma_eval_j[i] + gamma), j = 0..3, d_z[i] = prod_{r < i} num_r / den_r for i < padded_n
 * (d_z[0] = 1) and *d_wrap (one device scalar) = the product of all padded_n ratios: one iff (with overwhelming probability
 * over beta, gamma) the wire values are constant on sigma's cycles.  d_wire_values[j] (device) hold n_values <= padded_n
 * entries; rows >= n_values read as zero (the prover pads the witness with zeros).  A zero denominator ->
 * PG_ERR_NON_EXISTING_INVERSE; bad sizes or sigma entries -> PG_ERR_INVALID_ARGUMENT.  Synchronises `stream`. */
pg_status pg_permutation_product(pg_engine *e, uint64_t padded_n, const pg_scalar *const d_wire_values[4], uint64_t n_values,
                                 const uint64_t *d_sigma, const pg_scalar *omega, const pg_scalar k[4], const pg_scalar *beta,
                                 const pg_scalar *gamma, pg_scalar *d_z, pg_scalar *d_wrap, void *stream);

/* ---- NTTs over the scalar field: interpolation and evaluation of the composer's columns -----------------------------------
 * dusk-plonk 0.8's EvaluationDomain::{fft, ifft, coset_fft, coset_ifft} [DEP-RECALL] on n = 2^log2_n points (log2_n <= 32), in
 * place on n_cols columns of d_data (device, Montgomery form): column j is d_data[j * col_stride .. j * col_stride + n),
 * col_stride >= n.  Natural order in and out, outputs fully reduced:
 *   PG_NTT_FORWARD:        e_j = sum_i c_i omega^(ij)
 *   PG_NTT_INVERSE:        c_i = n^-1 sum_j e_j omega^(-ij)
 *   PG_NTT_COSET_FORWARD:  the forward transform of c_i g^i
 *   PG_NTT_COSET_INVERSE:  its exact inverse: the inverse transform, then times g^-i
 * omega: a primitive 2^log2_n-th root of unity (omega^(2^(log2_n - 1)) = -1; omega = 1 for log2_n = 0), e.g. pg_domain_generator;
 * coset_gen (g): nonzero, read only by the coset kinds (NULL otherwise; the Python layer's default is 7 [DEP-RECALL]).  The host
 * checks them and computes n^-1, omega^-1 and g^-1 itself.  Bad sizes, a stride below n, a NULL or misaligned pointer, an omega
 * of the wrong order or a zero g -> PG_ERR_INVALID_ARGUMENT with nothing launched.  Nothing on the device can fail, so the call
 * only enqueues on `stream` and does not synchronise.  Device memory the engine keeps for it (grow-only):
 * (2^L + n / 2^L) x 32 bytes, L = min(log2_n, 10), twice that for the coset kinds (64 MiB / 128 MiB at n = 2^31). */
enum { PG_NTT_FORWARD = 0, PG_NTT_INVERSE = 1, PG_NTT_COSET_FORWARD = 2, PG_NTT_COSET_INVERSE = 3 };
pg_status pg_ntt(pg_engine *e, pg_scalar *d_data, uint64_t n_cols, uint64_t col_stride, uint32_t log2_n, uint32_t kind,
                 const pg_scalar *omega, const pg_scalar *coset_gen, void *stream);

/* ---- the quotient polynomial and evaluations at a point: the prover's rounds 3 and 4 ------------------------------------
 * pg_quotient: dusk-plonk 0.8's quotient_poly::compute [DEP-RECALL] for the arithmetic gate, the public inputs and the copy
 * permutation, on n = 2^log2_n (log2_n <= 30; the inputs of 2^28 are the most one MI355X holds).  Every
 * input is a polynomial of n coefficients (device, Montgomery form), e.g. StandardComposer.prover_polynomials().  With
 * omega = omega_4n^4 (the generator of H), k = (k0..k3) the wire coset constants and x on the coset coset_gen * <omega_4n>:
 *   N(x) = q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c) + PI
 *        + alpha [ (a + beta k0 x + gamma)(b + beta k1 x + gamma)(c + beta k2 x + gamma)(d + beta k3 x + gamma) z(x)
 *                - (a + beta sigma1 + gamma)(b + beta sigma2 + gamma)(c + beta sigma3 + gamma)(d + beta sigma4 + gamma) z(omega x) ]
 *        + alpha^2 (z(x) - 1) L1(x),     L1(x) = (x^n - 1) / (n (x - 1))
 * d_t (4n scalars) gets the polynomial t of degree < 4n with t(x) = N(x) / (x^n - 1) on those 4n points, as t_lo | t_mid | t_hi |
 * t_4th (n coefficients each).  For a satisfied circuit with n >= 2, t (X^n - 1) = N exactly and deg t <= 4n - 5: the top four
 * coefficients of t_4th are zero.
 * d_scratch: PG_QUOTIENT_SCRATCH_COLS x n scalars the call overwrites (64 GiB at 2^28).  Bad sizes, a NULL (pi aside) or
 * misaligned pointer, an omega_4n whose order is not exactly 4n, coset_gen = 0 or coset_gen^(4n) = 1, a d_t or d_scratch that
 * overlaps an input or each other -> PG_ERR_INVALID_ARGUMENT with nothing launched.  Nothing on the device can fail, so the call
 * only enqueues on `stream`.  Device memory the engine keeps for it (grow-only): pg_ntt's tables for n, and one more table of
 * (2^L + n / 2^L) x 32 bytes, L = min(log2_n, 10) (8 MiB at 2^28). */
typedef struct pg_quotient_polys {
    const pg_scalar *w[4], *z, *sigma[4];
    const pg_scalar *q_m, *q_l, *q_r, *q_o, *q_4, *q_c, *q_arith;
    const pg_scalar *pi; /* NULL: the zero polynomial */
} pg_quotient_polys;     /* each: n coefficients, device, Montgomery form */
enum { PG_QUOTIENT_SCRATCH_COLS = 8 };
pg_status pg_quotient(pg_engine *e, uint32_t log2_n, const pg_quotient_polys *p, const pg_scalar *alpha, const pg_scalar *beta,
                      const pg_scalar *gamma, const pg_scalar *omega_4n, const pg_scalar k[4], const pg_scalar *coset_gen,
                      pg_scalar *d_t, pg_scalar *d_scratch, void *stream);
/* pg_quotient_blinded: the same quotient for blinded wire and permutation polynomials (the PLONK paper's rounds 1 and 2; DESIGN
 * section 3.17), which is what makes a proof zero-knowledge.  p->w[j] points at n + 2 coefficients, w_j = w_j0 + (b1 X + b0)(X^n - 1),
 * and p->z at n + 3, z = z0 + (b2 X^2 + b1 X + b0)(X^n - 1): plain coefficient arrays, rows n.. the blinders and the low rows less
 * them.  Every other input has n coefficients, as above.  N then has degree <= 5n + 6, and d_t gets 4n + 8 scalars: t_lo | t_mid |
 * t_hi | t_4th with t_4th of n + 8 rows, the last of them 0.  With T_i the coefficient 5n + i of N (i < 7) and t~ the polynomial of
 * degree < 4n with t~(x) = N(x) / (x^n - 1) on the 4n points, d_t[4n + i] = T_i, d_t[k] = t~[k] - coset_gen^(4n) T_k for k < 7 and
 * d_t[k] = t~[k] for the other k < 4n: for a satisfied circuit, exactly N / (X^n - 1).  The transforms stay n-point ones: one more
 * pointwise step per chunk adds x^n times the blinders' terms to the wires' and z's values, and one lane computes the T_i from the
 * top seven coefficients of the permutation products' factors.  With blinders of zero, rows 0..4n-1 are pg_quotient's.
 * 3 <= log2_n <= 30; d_scratch and every check as for pg_quotient, overlaps against the longer extents; the call only enqueues. */
pg_status pg_quotient_blinded(pg_engine *e, uint32_t log2_n, const pg_quotient_polys *p, const pg_scalar *alpha,
                              const pg_scalar *beta, const pg_scalar *gamma, const pg_scalar *omega_4n, const pg_scalar k[4],
                              const pg_scalar *coset_gen, pg_scalar *d_t, pg_scalar *d_scratch, void *stream);
/* pg_quotient_range: pg_quotient (blinded = 0) or pg_quotient_blinded (blinded != 0) with the range widget's term (DESIGN section
 * 3.19; pg_composer_range_gate):
 *   N(x) += q_range(x) [ alpha^3 delta(b - 4a) + alpha^4 delta(c - 4b) + alpha^5 delta(a(omega x) - 4c) ],  delta(f) = f (f-1)(f-2)(f-3)
 * d_q_range: n coefficients (device, Montgomery form), not blinded; NULL: exactly the launches, and the bytes, of the call it
 * generalises.  Otherwise one more n-point transform and one pointwise step per chunk (a, b, c and a(omega x) are resident), and,
 * blinded, the term's degree <= 5n + 3 adds to T_0 .. T_3 (one more lane-kernel).  Every check as for those calls; d_q_range must
 * not overlap d_t or d_scratch. */
pg_status pg_quotient_range(pg_engine *e, uint32_t log2_n, const pg_quotient_polys *p, const pg_scalar *d_q_range, int blinded,
                            const pg_scalar *alpha, const pg_scalar *beta, const pg_scalar *gamma, const pg_scalar *omega_4n,
                            const pg_scalar k[4], const pg_scalar *coset_gen, pg_scalar *d_t, pg_scalar *d_scratch, void *stream);
/* pg_poly_evaluate: d_out[j] = sum_{i < n} c_j[i] point^i for the n_cols columns c_j = d_coeffs + j * col_stride (device,
 * Montgomery form; 1 <= n <= 2^32, col_stride >= n; point^0 = 1, so point = 0 gives c_j[0]).  A bad n or stride, a NULL or
 * misaligned pointer, or a point not reduced below the modulus -> PG_ERR_INVALID_ARGUMENT with nothing launched; otherwise
 * the call only enqueues.  Device memory the engine keeps for it (grow-only): (257 + (n_cols + 1) ceil(n / 16384)) x 32 bytes. */
pg_status pg_poly_evaluate(pg_engine *e, const pg_scalar *d_coeffs, uint64_t n_cols, uint64_t col_stride, uint64_t n,
                           const pg_scalar *point, pg_scalar *d_out, void *stream);

/* ---- commitments: BLS12-381 G1 and the multi-scalar multiplication -------------------------------
 * pg_g1_affine: a point of G1 (y^2 = x^3 + 4 over the base field Fq, p = 0x1a0111ea...ffffaaab) in affine coordinates, each
 * coordinate 6 little-endian 64-bit limbs in Montgomery form (R = 2^384), fully reduced below p; (0, 0) is the identity.
 * 96 bytes; device arrays of them must be 16-byte aligned. */
typedef struct pg_g1_affine { uint64_t x[6], y[6]; } pg_g1_affine;
/* pg_msm: d_out[j] = sum_{i < n} s_j[i] P_i for the n_cols scalar columns s_j = d_scalars + j * col_stride (device, Montgomery
 * form, fully reduced) against the same n bases P_i = d_bases[i] (device).  Outputs are normalised affine points, so the
 * limbs do not depend on the order of summation.  1 <= n < 2^31, col_stride >= n.  Bases not on the curve are the caller's
 * problem: the sum is then meaningless (nothing is checked on the device).  n = 0, a stride below n, a NULL or misaligned
 * pointer, or d_out overlapping an input -> PG_ERR_INVALID_ARGUMENT with nothing launched; otherwise the call only enqueues.
 * Pippenger with 16 windows of signed 16-bit digits.  Device memory the engine keeps for it (grow-only): 16 n bytes of sort
 * keys and values, the sort's temporary storage, 2 ceil(n / 64) (4 + 192) bytes of partial bucket sums (and 1/32 of that
 * again), 16 (2^15 + 1) x 192 bytes of buckets and ~1 MB of per-window sums: about 5.6 GiB at n = 2^28. */
pg_status pg_msm(pg_engine *e, const pg_g1_affine *d_bases, const pg_scalar *d_scalars, uint64_t n, uint64_t n_cols,
                 uint64_t col_stride, pg_g1_affine *d_out, void *stream);
/* pg_msm_segmented: many independent small sums in one call:
 *   d_out[s * n_cols + j] = sum_{seg_off[s] <= i < seg_off[s + 1]} s_j[i] P_i        for s < n_segs, j < n_cols,
 * normalised affine points; an empty segment gives the identity (0, 0).  Bases, scalars, col_stride and alignment are as for
 * pg_msm.  seg_off is a HOST array of n_segs + 1 offsets with seg_off[0] = 0, non-decreasing, seg_off[n_segs] = n; it is
 * checked here and copied to the device (it is the caller's again when the call returns).  A bad seg_off, n = 0 with
 * n_segs > 0, n_cols = 0, a stride below n, n x n_cols >= 2^31 (or n_segs x n_cols >= 2^31), a NULL or misaligned pointer, or
 * d_out overlapping an input -> PG_ERR_INVALID_ARGUMENT with nothing launched; n_segs = 0 does nothing and is PG_OK;
 * otherwise the call only enqueues -- behind one host wait when the engine's previous pg_msm_segmented is still pending: seg_off
 * is staged in one pinned buffer, which is rewritten only after the copy that last read it has left.
 * Every product s_j[i] P_i is a scalar multiplication on a lane of its own: 86 fixed windows of signed 3-bit digits over a
 * table 2P, 3P, 4P in LDS (255 doublings and up to 86 complete additions: about 3 500 Fq products per point and column,
 * whatever the scalar).  One wave per (segment, column) then sums the segment's products -- a segment of any length is
 * correct, only short ones are fast: one large sum is pg_msm's -- and one pass normalises all the sums.  Device memory the
 * engine keeps for it (grow-only): 192 bytes x n x n_cols of products, 192 bytes x n_segs x n_cols of sums, 8 (n_segs + 1)
 * bytes of offsets (and as many of pinned host memory). */
pg_status pg_msm_segmented(pg_engine *e, const pg_g1_affine *d_bases, const pg_scalar *d_scalars, uint64_t n, uint64_t n_cols,
                           uint64_t col_stride, const uint64_t *seg_off /* HOST, n_segs + 1 */, uint64_t n_segs,
                           pg_g1_affine *d_out /* [n_segs][n_cols] */, void *stream);
/* pg_srs_setup: d_out[i] = tau^i * base for i < n (1 <= n <= 2^32), base == NULL meaning the generator G.  This is
 * dusk-plonk's PublicParameters::setup `powers_of_g` with the secret tau chosen by the caller: INSECURE, for development
 * and tests only (whoever knows tau can forge proofs).  tau (host, Montgomery form) = 0 or not reduced, a base (host) that
 * is the identity or not reduced, a NULL or misaligned d_out -> PG_ERR_INVALID_ARGUMENT.  Enqueues only.  Device memory the
 * engine keeps for it (grow-only): 2.3 MiB of fixed-base tables and 384 MiB for a chunk of 2^21 points. */
pg_status pg_srs_setup(pg_engine *e, const pg_scalar *tau, const pg_g1_affine *base, uint64_t n, pg_g1_affine *d_out, void *stream);
/* pg_g1_to_compressed (host only): the 48-byte zcash / dusk-bls12_381 encoding of `count` points, out[48 i ...]: x big-endian,
 * bit 7 of the first byte set (compressed), bit 6 for the identity (then every other bit is 0), bit 5 when y > (p - 1) / 2.
 * NULL pointers with count > 0, or coordinates not reduced -> PG_ERR_INVALID_ARGUMENT. */
pg_status pg_g1_to_compressed(const pg_g1_affine *in, uint64_t count, uint8_t *out);

/* ---- G1 ingestion: decompression, membership and compression in batches ----------------------------
 * What a commit key made elsewhere needs before it can be trusted: every 48-byte encoding decoded, every point shown to be on
 * the curve and of order dividing r.  One status byte per point: */
enum {
    PG_G1_OK = 0,
    PG_G1_BAD_ENCODING = 1,    /* the compressed bit clear, an identity encoding other than c0 00 .. 00, or x >= p */
    PG_G1_NOT_ON_CURVE = 2,    /* x^3 + 4 has no square root (decompression) / y^2 != x^3 + 4 (check) */
    PG_G1_NOT_IN_SUBGROUP = 3, /* on the curve, but r P != O */
    PG_G1_NOT_REDUCED = 4      /* pg_g1_check: limbs at or above p (pg_msm refuses such points too) */
};
/* pg_g1_decompress: d_out[i] = the point of d_in[48 i .. 48 i + 47] (device, the encoding of pg_g1_to_compressed), for i < n:
 * y = (x^3 + 4)^((p + 1) / 4) with the sign of bit 5; with check_subgroup != 0 also the membership test (the endomorphism
 * test phi(P) = [-u^2] P, which implies r P = O).  d_status[i] (device, n bytes) is the point's PG_G1_* value; a point whose
 * status is not PG_G1_OK is written as the identity, never as garbage.  *d_first_bad (device, one uint64) = the smallest i
 * with d_status[i] != PG_G1_OK, n if there is none.  1 <= n <= 2^32; d_in and d_out 16-byte aligned, d_first_bad 8-byte.
 * pg_g1_check: the same statuses for n points already in limbs (PG_G1_NOT_REDUCED, then the curve, then the subgroup; the
 * identity (0, 0) is PG_G1_OK); writes no point.
 * pg_g1_compress: d_out[48 i ...] = the encoding of d_points[i]; the points' limbs must be reduced (those of
 * pg_g1_decompress, pg_msm and pg_srs_setup are), nothing is checked on the device.
 * n out of range, a NULL or misaligned pointer, or an output overlapping an input or another output ->
 * PG_ERR_INVALID_ARGUMENT with nothing launched; otherwise the calls only enqueue.  One lane per point, about 541 Fq products
 * to decode and 1 280 to test membership; they keep no device memory. */
pg_status pg_g1_decompress(pg_engine *e, const uint8_t *d_in, uint64_t n, int check_subgroup, pg_g1_affine *d_out, uint8_t *d_status,
                           uint64_t *d_first_bad, void *stream);
pg_status pg_g1_check(pg_engine *e, const pg_g1_affine *d_points, uint64_t n, uint8_t *d_status, uint64_t *d_first_bad, void *stream);
pg_status pg_g1_compress(pg_engine *e, const pg_g1_affine *d_points, uint64_t n, uint8_t *d_out, void *stream);
/* pg_g1_from_compressed, pg_g1_check_host (host only): the same routines on the host, one point after the other, for `count`
 * encodings / points; pg_g1_from_compressed always tests membership.  They need no GPU.  NULL pointers with count > 0 ->
 * PG_ERR_INVALID_ARGUMENT; a bad point is reported in status[i], not by the return value. */
pg_status pg_g1_from_compressed(const uint8_t *in, uint64_t count, pg_g1_affine *out, uint8_t *status);
pg_status pg_g1_check_host(const pg_g1_affine *in, uint64_t count, uint8_t *status);

/* ---- the verifier's sides from proof bytes, a batch at a time --------------------------------------
 * What lies between a proof's 1040 bytes (11 commitments of 48 bytes, 16 evaluations of 32) and the input of
 * pg_msm_segmented: the Fiat-Shamir transcript (Merlin over STROBE-128 over Keccak-f[1600]), the seven challenges, the
 * verifier's scalar algebra and the table of coefficients -- one proof per lane.  The KZG check of a proof is
 *     e(sum_k a_k P_k, [tau]_2) e(sum_k b_k P_k, [1]_2) = 1
 * over a fixed table of PG_PLONK_SIDES_ROWS = 23 rows (P_k, a_k, b_k) per proof:
 *    0..10  the proof's a, b, c, d, z, t_1, t_2, t_3, t_4, w_z, w_zw commitments
 *   11..21  the key's q_m, q_l, q_r, q_o, q_4, q_c, q_arith, left_sigma, right_sigma, out_sigma, fourth_sigma
 *       22  the generator g of the opening key
 * Equal points are not merged: a point that stands in two rows carries two scalars, and the sums are the same.
 *
 * pg_plonk_key: what the routine needs of a (verifier key, transcript label) pair.  The transcript does not start from
 * scratch: `state`, `pos`, `pos_begin`, `cur_flags` are the STROBE-128 state as it stands after the label, the circuit's domain
 * separator and the key's 15 commitments (the host computes that once per key and label; every operation that follows
 * begins afresh, so cur_flags is carried but not read).  pos <= 165, pos_begin <= 166, log2_n <= 32; omega is the generator
 * of the 2^log2_n domain, in Montgomery form; the points are trusted (nothing tests them).  1392 bytes. */
#define PG_PLONK_PROOF_BYTES 1040
#define PG_PLONK_SIDES_ROWS 23
typedef struct pg_plonk_key {
    uint8_t state[200];
    uint8_t pos, pos_begin, cur_flags, log2_n;
    uint32_t reserved;
    pg_scalar omega;
    pg_g1_affine points[11]; /* q_m, q_l, q_r, q_o, q_4, q_c, q_arith, left_sigma, right_sigma, out_sigma, fourth_sigma */
    pg_g1_affine g;
} pg_plonk_key;
/* One status byte and one `where` byte per proof.  The tests run in the order key, commitments, evaluations, public inputs,
 * xi^n; the first that fails is reported.  1..4 are the PG_G1_* status of the first bad commitment (decoded with the
 * membership test), `where` its index among the 11; otherwise: */
enum {
    PG_SIDES_OK = 0,
    PG_SIDES_BAD_EVALUATION = 5,   /* an evaluation's 32 bytes are not below r; `where` is its index among the 16 */
    PG_SIDES_XI_IN_DOMAIN = 6,     /* xi^n = 1: Z_H(xi) = 0, nothing to divide by */
    PG_SIDES_BAD_PUBLIC_INPUT = 7, /* a public-input row >= n, or a value whose limbs are not below r */
    PG_SIDES_BAD_KEY = 8           /* d_key_index[i] >= n_keys, or a key record with pos, pos_begin or log2_n out of range */
};
/* pg_plonk_sides: for proof i < n (d_proofs[1040 i ..], device, 16-byte aligned) under the key d_keys[d_key_index[i]]
 * (d_key_index == NULL: key 0 for all) with the public inputs rows d_pi_rows[k], values d_pi_vals[k] (Montgomery form) for
 * d_pi_off[i] <= k < d_pi_off[i + 1] (d_pi_off == NULL: none, and the two arrays are not read; else all three non-NULL).
 * d_pi_off is on the device, so nothing can check it here: it MUST be non-decreasing, and d_pi_rows and d_pi_vals must hold
 * d_pi_off[n] entries -- the kernel reads every k the offsets name, and an offset past the arrays is an out-of-bounds read (a
 * decreasing pair reads nothing for that proof).  The call writes
 *   d_bases[23 i + k] = P_k,   d_scalars[23 i + k] = a_k,   d_scalars[col_stride + 23 i + k] = b_k,
 * the layout pg_msm_segmented takes with n_cols = 2 and seg_off[s] = 23 s, and d_status[i], d_where[i].  A rejected proof's
 * 23 rows are identities and zeros, never garbage: its two sums are then the identity and its pairing check PASSES, so the
 * verdict on proof i is  d_status[i] == PG_SIDES_OK  AND  the pairing check.  A key index >= n_keys is a per-proof rejection
 * (PG_SIDES_BAD_KEY), not an argument error: the indices are on the device and the call only enqueues.
 * e, a pointer NULL or misaligned (16 bytes for proofs, keys, bases, scalars and values, 8 for offsets and rows, 4 for key
 * indices), n x 23 >= 2^31, n_keys = 0, col_stride < 23 n, an output overlapping another output or the proofs, keys, key
 * indices or offsets -> PG_ERR_INVALID_ARGUMENT with nothing launched; n = 0 is PG_OK and does nothing.  Two launches: the
 * 11 n commitments decoded one per lane (about 1 820 Fq products each), then one lane per proof: 14 or 15 permutations, 112 +
 * log2 n products in Fr plus at most 2 log2 n + 4 per public input, one inversion.  Device memory the engine keeps for it (grow-only):
 * 11 n bytes.
 * pg_plonk_sides_host (host only): the same routine on the host, one proof after the other, every pointer a host pointer
 * (8-byte aligned where its elements are words); needs no GPU. */
pg_status pg_plonk_sides(pg_engine *e, const uint8_t *d_proofs /* n x 1040 bytes */, uint64_t n, const pg_plonk_key *d_keys,
                         uint64_t n_keys, const uint32_t *d_key_index /* [n], NULL = all 0 */,
                         const uint64_t *d_pi_off /* [n + 1], NULL = no public inputs */, const uint64_t *d_pi_rows,
                         const pg_scalar *d_pi_vals, pg_g1_affine *d_bases /* [23 n] */, pg_scalar *d_scalars /* [2][col_stride] */,
                         uint64_t col_stride, uint8_t *d_status, uint8_t *d_where, void *stream);
pg_status pg_plonk_sides_host(const uint8_t *proofs, uint64_t n, const pg_plonk_key *keys, uint64_t n_keys, const uint32_t *key_index,
                              const uint64_t *pi_off, const uint64_t *pi_rows, const pg_scalar *pi_vals, pg_g1_affine *bases,
                              pg_scalar *scalars, uint64_t col_stride, uint8_t *status, uint8_t *where);

/* pg_plonk_range_sides: pg_plonk_sides with the range widget's term of r(X) (DESIGN sections 3.19 and 3.21;
 * pg_composer_range_gate, pg_composer_interval_gate), for proofs of circuits that carry range_gate or interval_gate items.  The
 * table has PG_PLONK_RANGE_SIDES_ROWS = 24 rows per proof: rows 0..22 are pg_plonk_sides' -- the same points and the same two
 * scalars -- and
 *       23  the key's q_range with a = 0 and b = -v rho_range,
 *           rho_range = alpha^3 delta(b - 4a) + alpha^4 delta(c - 4b) + alpha^5 delta(a_w - 4c),  delta(f) = f (f-1)(f-2)(f-3)
 * over the proof's evaluations a_eval, b_eval, c_eval and a_next_eval (19 more products in Fr per proof).
 * pg_plonk_range_key: a pg_plonk_key -- its first 1392 bytes are one, field for field -- followed by the key's q_range
 * commitment; 1488 bytes.  A record whose q_range is the identity gets row 23 = (identity, 0, 0) and with it the two sums that
 * pg_plonk_sides gives its first 1392 bytes: keys with and without the widget can share one call.  The transcript is
 * pg_plonk_sides': the seed has absorbed all 15 commitments of the key, q_range among them.
 * The call writes d_bases[24 i + k], d_scalars[24 i + k] and d_scalars[col_stride + 24 i + k], the layout pg_msm_segmented
 * takes with seg_off[s] = 24 s; a rejected proof's 24 rows are identities and zeros.  Every argument, every check, d_status
 * and d_where as for pg_plonk_sides, with the row bounds n x 24 < 2^31 and col_stride >= 24 n; the same two launches (the
 * second a kernel of its own) and the same 11 n bytes of device memory.  Like pg_plonk_sides the call is asynchronous: both
 * launches are ordered on `stream` behind its earlier work, the host does not wait for them, and the engine's workspace is
 * handed from the stream of its previous call to this one.
 * pg_plonk_range_sides_host (host only): the same routine on the host, as pg_plonk_sides_host is pg_plonk_sides'. */
#define PG_PLONK_RANGE_SIDES_ROWS 24
typedef struct pg_plonk_range_key {
    uint8_t state[200];
    uint8_t pos, pos_begin, cur_flags, log2_n;
    uint32_t reserved;
    pg_scalar omega;
    pg_g1_affine points[11]; /* as in pg_plonk_key */
    pg_g1_affine g;
    pg_g1_affine q_range;
} pg_plonk_range_key;
pg_status pg_plonk_range_sides(pg_engine *e, const uint8_t *d_proofs /* n x 1040 bytes */, uint64_t n,
                               const pg_plonk_range_key *d_keys, uint64_t n_keys, const uint32_t *d_key_index /* [n], NULL = all 0 */,
                               const uint64_t *d_pi_off /* [n + 1], NULL = no public inputs */, const uint64_t *d_pi_rows,
                               const pg_scalar *d_pi_vals, pg_g1_affine *d_bases /* [24 n] */,
                               pg_scalar *d_scalars /* [2][col_stride] */, uint64_t col_stride, uint8_t *d_status, uint8_t *d_where,
                               void *stream);
pg_status pg_plonk_range_sides_host(const uint8_t *proofs, uint64_t n, const pg_plonk_range_key *keys, uint64_t n_keys,
                                    const uint32_t *key_index, const uint64_t *pi_off, const uint64_t *pi_rows, const pg_scalar *pi_vals,
                                    pg_g1_affine *bases, pg_scalar *scalars, uint64_t col_stride, uint8_t *status, uint8_t *where);

/* ---- openings: the prover's round 5 ---------------------------------------------------------------
 * Both calls take n_cols (1..32) columns p_j = d_cols[j] of n coefficients each (device, Montgomery form, 1 <= n <= 2^32) as a
 * HOST array of device pointers, which may repeat (one column can carry two weights), and n_cols host weights mu[j]; f is
 * sum_j mu_j p_j.
 * pg_poly_open: dusk-plonk 0.8's CommitKey::compute_aggregate_witness followed by Polynomial::ruffini [DEP-RECALL] (mu_j = v^j
 * there; here mu may also carry the xi^(jn) factors that assemble t from its parts).  d_witness[i] = q_i for i < n - 1, where
 * f = q (X - point) + f(point): q_{n-2} = f_{n-1}, q_{i-1} = f_i + point q_i; d_witness[n - 1] = 0, so the witness is a plain
 * n-coefficient column CommitKey.commit takes as is.  d_value (device, one scalar) = f(point).
 * pg_poly_combine: d_out = f (n coefficients), nothing divided.
 * A NULL or misaligned pointer, n_cols or n out of range, a weight or point not reduced below the modulus, an output that
 * overlaps an input column (or d_value overlapping d_witness) -> PG_ERR_INVALID_ARGUMENT with nothing launched; otherwise the
 * calls only enqueue on `stream`.  Device memory the engine keeps for pg_poly_open (grow-only): ceil(n / 2048) x 32 bytes of
 * tile totals (4 MiB at n = 2^28).  pg_poly_combine keeps none. */
pg_status pg_poly_open(pg_engine *e, const pg_scalar *const *d_cols, const pg_scalar *mu, uint64_t n_cols, uint64_t n,
                       const pg_scalar *point, pg_scalar *d_witness, pg_scalar *d_value, void *stream);
pg_status pg_poly_combine(pg_engine *e, const pg_scalar *const *d_cols, const pg_scalar *mu, uint64_t n_cols, uint64_t n,
                          pg_scalar *d_out, void *stream);

/* ---- verification: BLS12-381 G2 on the host and the pairing check on the device ---------------------
 * pg_g2_affine: a point of G2, the order-r subgroup of the twist y^2 = x^3 + 4 (1 + u) over Fq2 = Fq[u] / (u^2 + 1), in affine
 * coordinates x.c0, x.c1, y.c0, y.c1, each 6 little-endian 64-bit limbs in Montgomery form, fully reduced; all zero is the
 * identity.  192 bytes.  G2 arithmetic is host-only: it happens once per key, never per proof. */
typedef struct pg_g2_affine { uint64_t x[12], y[12]; } pg_g2_affine;
/* a G2 point prepared for pairings: the 68 line functions of the ate Miller loop over it, on the engine's device */
typedef struct pg_g2_prepared pg_g2_prepared;
/* pg_g2_mul (host only): *out = k * p, p == NULL meaning the generator of G2 [DEP-RECALL]; k in Montgomery form.  Affine
 * double-and-add, a few milliseconds.  NULL k or out, k or a coordinate not reduced, p not on the twist ->
 * PG_ERR_INVALID_ARGUMENT.  Membership of the order-r subgroup is not tested: (r - 1) p == -p is that test. */
pg_status pg_g2_mul(const pg_g2_affine *p, const pg_scalar *k, pg_g2_affine *out);
/* pg_g2_to_compressed (host only): the 96-byte zcash / dusk-bls12_381 encoding of `count` points, out[96 i ...]: x.c1 then x.c0,
 * big-endian; in the first byte bit 7 set (compressed), bit 6 for the identity (then every other bit is 0), bit 5 when y is
 * the larger of (y, -y), compared by c1 first and then by c0.  NULL pointers with count > 0, or coordinates not reduced ->
 * PG_ERR_INVALID_ARGUMENT. */
pg_status pg_g2_to_compressed(const pg_g2_affine *in, uint64_t count, uint8_t *out);
/* pg_g2_prepare: runs the doubling and addition steps of the ate loop over |x| = 0xd201000000010000 on the host and uploads
 * the 68 lines (2 Fq2 each: 13 056 bytes) to the engine's device; synchronous.  *out is released with
 * pg_g2_prepared_destroy, before the engine.  q must be on the twist and of order r (the first is checked, the second is the
 * caller's duty); the identity, a point off the twist, coordinates not reduced or a NULL -> PG_ERR_INVALID_ARGUMENT. */
pg_status pg_g2_prepare(pg_engine *e, const pg_g2_affine *q, pg_g2_prepared **out);
void pg_g2_prepared_destroy(pg_g2_prepared *p);
/* pg_pairing_check: d_ok[i] = 1 if prod_{j < n_pairs} e(P_ij, Q_j) == 1, else 0, for the n_checks rows P_i of
 * d_points[n_checks][n_pairs] (device; on the curve and in G1 -- nothing is checked on the device; an identity P contributes
 * 1) against the same n_pairs prepared points (a HOST array of handles).  Per check: one Miller loop that accumulates all
 * pairs into one value, one final exponentiation.  1 <= n_pairs <= 8 (the points of a check are staged in LDS that the final
 * exponentiation reuses; a KZG check needs 2); n_checks = 0 does nothing.  Six lanes share a check and a workgroup of 252
 * carries 42, so n_checks = 1 is one workgroup: a single check is bound by latency (about 9 000 dependent Fq products).
 * NULL or misaligned pointers, n_pairs out of range, n_checks > 2^31, a handle of another device -> PG_ERR_INVALID_ARGUMENT
 * with nothing launched; otherwise the call only enqueues.  Keeps no device memory.
 * pg_pairing_gt: the GT values themselves, d_gt[i] = 72 limbs: the six Fq2 coefficients over w^0 .. w^5 (w^6 = 1 + u) of
 * (prod_j e(P_ij, Q_j))^3, where e is the ate pairing with the plain final power (p^12 - 1) / r -- the hard part's addition
 * chain computes the cube, which is 1 exactly when the product is.  For tests and for callers that compare values. */
pg_status pg_pairing_check(pg_engine *e, const pg_g1_affine *d_points, const pg_g2_prepared *const *prepared, uint64_t n_checks,
                           uint64_t n_pairs, uint8_t *d_ok, void *stream);
pg_status pg_pairing_gt(pg_engine *e, const pg_g1_affine *d_points, const pg_g2_prepared *const *prepared, uint64_t n_checks,
                        uint64_t n_pairs, uint64_t *d_gt, void *stream);

/* ---- multi-GPU: shards, packed chunks, the all-gather (BASELINE.json config 5) -------------
 * The reference has no counterpart: it is single-threaded (`&mut StandardComposer`, src/range.rs:27-32).  What is
 * sharded is the loop  for w in witnesses { allocate; range_check }  of tests/range_gadgets_tests.rs:29-44: items are
 * independent and item i owns rows [gate_base + i*G, +G) and variables [var_base + i*V, +V), so rank r of P emits its
 * contiguous range [lo, hi) straight at its final global numbering -- no exchange is needed to place anything.  One
 * process per GPU; the host (the Rust host of north_star, or Python) calls the same entry points on every rank. */
typedef struct pg_shard {
    uint32_t rank, world;
    uint64_t lo, hi;              /* this rank's items of the whole batch: [lo, hi); the first total % world ranks get one more */
    uint64_t gate_base, var_base; /* global number of the shard's first row / first variable */
    uint64_t n_gates, n_vars;     /* rows / variables the shard emits */
} pg_shard;
pg_status pg_shard_range(uint64_t total, uint32_t rank, uint32_t world, uint64_t *lo, uint64_t *hi);
pg_status pg_range_check_shard_layout(const pg_scalar *min_range, const pg_scalar *max_range, uint64_t total, uint32_t rank,
                                      uint32_t world, uint64_t gate_base, uint64_t var_base, pg_shard *out);
/* pg_range_check_batch on this rank's shard of a `total`-item batch whose first row / variable are (gate_base,
 * var_base): d_witness_local holds the hi - lo witnesses of the shard, `out` buffers sized by the shard layout.
 * No communication.  `shard` (may be NULL) receives the placement. */
pg_status pg_range_check_sharded_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range,
                                       const pg_scalar *d_witness_local, uint64_t total, uint32_t rank, uint32_t world,
                                       uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                       pg_variable *d_result_vars /* may be NULL */, pg_shard *shard, void *stream);

/* A packed chunk: the nine arrays of one call back to back in ONE buffer (offsets in 8-byte words, every section
 * starting on a 128-byte line of a buffer that does), so that a chunk is a single collective.  pg_columns_in_packed gives the pg_columns view to emit into. */
typedef struct pg_packed {
    uint64_t q_words[5], w_words[3], var_words; /* offsets of q_m..q_c, w_l..w_o, var_values */
    uint64_t total_words, n_gates, n_vars;
} pg_packed;
pg_status pg_packed_layout(uint64_t n_gates, uint64_t n_vars, pg_packed *out);
pg_status pg_columns_in_packed(void *d_packed, uint64_t n_gates, uint64_t n_vars, pg_columns *out);

/* The communicator: RCCL over xGMI, bound at run time (dlsym in the process, then dlopen of librccl.so.1; PG_RCCL_LIB
 * overrides) -- the library itself does not link RCCL.  Rank 0 calls pg_comm_unique_id and hands the 128 bytes to the
 * other ranks out of band (the host's own channel: a file, a socket, MPI, torch.distributed); every rank then calls
 * pg_comm_create with the same id (collective: returns when all `world` ranks have joined).  A host that already owns
 * an ncclComm_t passes it to pg_comm_adopt instead (not destroyed by pg_comm_destroy). */
#define PG_COMM_ID_BYTES 128
typedef struct pg_comm pg_comm;
pg_status pg_comm_unique_id(uint8_t id[PG_COMM_ID_BYTES]);
/* path of the RCCL the library bound ("" if none was found): inside a PyTorch process it must be PyTorch's own copy */
const char *pg_comm_library(void);
pg_status pg_comm_create(pg_engine *e, const uint8_t id[PG_COMM_ID_BYTES], uint32_t rank, uint32_t world, pg_comm **out);
pg_status pg_comm_adopt(pg_engine *e, void *nccl_comm, pg_comm **out);
void pg_comm_destroy(pg_comm *c);
uint32_t pg_comm_rank(const pg_comm *c);
uint32_t pg_comm_world(const pg_comm *c);
/* "a single RCCL all-gather of the emitted gate columns" (north_star), enqueued on `stream` after the emission:
 *   pg_allgather_bytes    d_recv[r * bytes_per_rank ..] = rank r's d_send (one ncclAllGather; a packed chunk, a variable
 *                         table, or the 16 bytes of (rows, variables) totals a ragged sharded batch exchanges);
 *   pg_allgather_columns  the nine arrays of equal-sized shards, one grouped launch; rank order == witness order, so
 *                         every gathered column is the whole batch's column (n_gates / n_vars: per rank). */
pg_status pg_allgather_bytes(pg_comm *c, const void *d_send, void *d_recv, uint64_t bytes_per_rank /* multiple of 8 */,
                             void *stream);
pg_status pg_allgather_columns(pg_comm *c, const pg_columns *local, uint64_t n_gates, uint64_t n_vars,
                               const pg_columns *gathered, void *stream);

/* BASELINE config 5 as ONE object: the chunked gather pipeline.  2^23 x 223 KB = 1.87 TB fits no GPU, so a sharded batch is
 * streamed in chunks of `chunk` witnesses per rank: chunk k + 1 is emitted on the caller's stream while chunk k is in
 * ncclAllGather on the pipeline's communication stream (two slots, events between the streams).  Numbering: rank r's
 * item i is item r * total_per_rank + i of the whole batch (contiguous witness shards).
 *   variables_only = 0  every rank's packed chunk travels (all nine arrays back to back, pg_packed_layout): one collective
 *                       of 223 KB per witness;
 *   variables_only = 1  only the variable tables travel (33 KB per witness); the other ranks' selectors and wire indices --
 *                       a function of the public bounds and the numbering -- are regenerated locally
 *                       (pg_range_check_structure_batch).
 * `consume` is called on the host, once per chunk and in order, when the chunk is complete for `stream`: parts[r] are the
 * nine arrays of rank r's chunk (device pointers owned by the pipeline, n_gates rows / n_vars variables each); whatever
 * the callback enqueues on `stream` reads them safely, and they are overwritten two chunks later.  The communicator must
 * outlive every run of the pipeline (not its destruction).  The reference has no
 * counterpart (one composer, one thread: src/range.rs:27-32); the shape is BASELINE.json config 5's. */
typedef struct pg_gather_pipeline pg_gather_pipeline;
typedef void (*pg_chunk_consumer)(void *user, uint64_t chunk_index, uint32_t world, const pg_columns *parts, uint64_t n_gates,
                                  uint64_t n_vars, void *stream);
pg_status pg_range_check_gather_pipeline_create(pg_comm *c, const pg_scalar *min_range, const pg_scalar *max_range,
                                                uint64_t chunk, uint32_t variables_only, pg_gather_pipeline **out);
/* bytes one rank puts on the links per chunk */
uint64_t pg_range_check_gather_pipeline_bytes_per_chunk(const pg_gather_pipeline *p);
pg_status pg_range_check_gather_pipeline_run(pg_gather_pipeline *p, const pg_scalar *d_witness_local,
                                             uint64_t total_per_rank /* a multiple of chunk */, uint64_t gate_base,
                                             uint64_t var_base, pg_chunk_consumer consume /* may be NULL */, void *user,
                                             void *stream);
void pg_range_check_gather_pipeline_destroy(pg_gather_pipeline *p);

/* Ragged sharded batches (one public bound per item: rows per item differ) have ONE real exchange step: every rank plans
 * its contiguous shard, the 16 bytes of (rows, variables) totals are all-gathered, and an exclusive prefix sum over the
 * ranks gives each rank the global numbering of its first row and variable.
 *   pg_max_bound_ragged_sharded_plan   plan + exchange; `shard` receives this rank's placement (gate_base / var_base
 *                                      already global, n_gates / n_vars its totals); gates_per_rank / vars_per_rank
 *                                      ([world] each, may be NULL) every rank's totals.  Synchronises `stream`.
 *   pg_max_bound_ragged_sharded_batch  the same followed by the emission (pg_max_bound_ragged_batch) at that numbering, for
 *                                      callers whose `out` holds the worst case (515 rows, 517 variables per item). */
pg_status pg_max_bound_ragged_sharded_plan(pg_comm *c, const pg_scalar *d_max_range_local, uint64_t batch_local,
                                           uint32_t *d_num_bits, uint64_t *d_row_off, uint64_t *d_var_off, uint64_t gate_base,
                                           uint64_t var_base, pg_shard *shard, uint64_t *gates_per_rank, uint64_t *vars_per_rank,
                                           void *stream);
pg_status pg_max_bound_ragged_sharded_batch(pg_comm *c, const pg_scalar *d_max_range_local, const pg_scalar *d_witness_local,
                                            uint64_t batch_local, uint32_t *d_num_bits, uint64_t *d_row_off, uint64_t *d_var_off,
                                            uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                            pg_variable *d_result_vars /* may be NULL */, pg_shard *shard, void *stream);

/* ---- where to put the columns ---------------------------------------------
 * pg_columns is nine device pointers and the library writes where it is told; on MI355X it matters where.  The emitters write
 * the same row of the five selector columns at once, and five such streams inside a few GiB of physical memory run 10-18 %
 * slower than five streams tens of GiB apart.  Columns of tens of GB each lie that far apart by
 * themselves; for a smaller circuit, allocate ONE block of *total_bytes and put the arrays at the offsets this call returns:
 * q_m, q_l, q_r, q_o, q_c `stride_bytes` apart (rounded up to 2 MiB; at least a column's own size), then w_l, w_r, w_o and the
 * variable table back to back behind q_c -- of the layouts measured the best (profiles/NOTES_r04.md section 7).  offsets[] in
 * the order of pg_columns' fields, every one a multiple of 2 MiB; the block itself should start on a 2-MiB boundary too (any
 * large hipMalloc does).  24 GiB is what bench.py's fused-mix configuration uses.  Host arithmetic only. */
pg_status pg_columns_slab_layout(uint64_t n_gates, uint64_t n_vars, uint64_t stride_bytes, uint64_t offsets[9],
                                 uint64_t *total_bytes);

/* ---- diagnostics ----------------------------------------------------------
 * Bare store streams, the comparison points bench.py measures in the same process as every workload (SURVEY.md section
 * 8d; `roofline.bare_fill` of its line).
 * pg_fill_columns: the emitters' store stream with nothing behind it -- a workgroup owns a tile of `rows_per_tile`
 * consecutive rows (0: 32768; a multiple of 8) and sweeps the five selector columns in lock step, then the three wire columns,
 * then its share of the variable table, 16 B per lane, one constant.  On the arrays a workload writes it is that workload's
 * store ceiling on those arrays (where lock-step streams lie decides 10-18 % on MI355X).  All nine
 * pointers 16-byte aligned.
 * pg_fill_bytes: one buffer.  streams = 1..16: written as that many equal parts advanced together by long-lived
 * workgroups; streams = 0: one short-lived workgroup per 8 KiB, two resident per CU (one moving window of a few MiB:
 * the shape that reaches 7.1-7.2 TB/s wherever the buffer lies). */
pg_status pg_fill_columns(pg_engine *e, const pg_columns *out, uint64_t n_gates, uint64_t n_vars, uint64_t rows_per_tile,
                          uint64_t pattern, void *stream);
pg_status pg_fill_bytes(pg_engine *e, void *d_dst /* 16-byte aligned */, uint64_t bytes /* multiple of 16 */,
                        uint32_t streams, uint64_t pattern, void *stream);

#ifdef __cplusplus
}
#endif
#endif
