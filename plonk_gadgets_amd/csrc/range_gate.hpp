// range_gate.hpp -- the quad-accumulator range widget on the composer's THREE wires: the gadget
// descriptor of range_gate(witness, num_bits) for the streaming writer (emit.hpp), the kernel that writes q_range = 1 on its
// rows into a materialized column, and the kernel that checks its statement.
//
// num_bits even, 2 <= num_bits <= 254 (4^127 < r: an accumulator chain cannot wrap).  k = num_bits / 2 quads, g = ceil(k / 3)
// widget rows, pad = 3g - k, v = the canonical integer of the witness's value.  Positions p = 0 .. 3g:
//   P(p) = zero_var                                         p <= pad
//   P(p) = first_var + (p - pad - 1), value v >> 2 (3g - p)  pad < p < 3g      (k - 1 new Variables)
//   P(3g) = the witness Variable itself
// Rows (w_l, w_r, w_o), every arithmetic selector 0 (the arithmetic gate is vacuous on them):
//   row i < g:  (P(3i), P(3i+1), P(3i+2))     q_range = 1
//   row g:      (P(3g), zero_var, zero_var)   q_range = 0
// A row with q_range = 1 states that each of b - 4a, c - 4b and a_next - 4c lies in {0, 1, 2, 3}: P(0) = 0 and 3g quads make
// P(3g) < 4^k.  An out-of-range witness still gets all its rows; its first accumulator is >= 4, so the item's row 0 fails.
// q_range is no column of the composer: the rows are remembered as segments (first row, items, g) on the host and written by
// range_patch_kernel when the columns are materialized.
#pragma once

#include "composer_cols.hpp"
#include "emit.hpp"

namespace pg {

// c >> s for a canonical integer, s in [0, 255]: named limbs and selects only (a limb array indexed by the shift goes to scratch)
PG_HD Fr raw_shr(const Fr &c, uint32_t s) {
    uint64_t l0 = c.l[0], l1 = c.l[1], l2 = c.l[2], l3 = c.l[3];
    if (s & 128) { l0 = l2; l1 = l3; l2 = 0; l3 = 0; }
    if (s & 64) { l0 = l1; l1 = l2; l2 = l3; l3 = 0; }
    const uint32_t b = s & 63;
    if (b) {
        l0 = (l0 >> b) | (l1 << (64 - b));
        l1 = (l1 >> b) | (l2 << (64 - b));
        l2 = (l2 >> b) | (l3 << (64 - b));
        l3 >>= b;
    }
    return Fr{{l0, l1, l2, l3}};
}

// the widget's shape for num_bits (the comment above): what the host sizes a call by and the Args below are filled from
struct WidgetShape {
    uint32_t k, g, pad;  // quads, widget rows, leading positions that are zero_var beside P(0)
    constexpr uint32_t rows() const { return g + 1; }  // of one widget: its g rows and the terminal row
};
constexpr WidgetShape widget_shape(uint64_t num_bits) {
    const uint32_t k = (uint32_t)(num_bits / 2), g = (k + 2) / 3;
    return WidgetShape{k, g, 3 * g - k};
}
// num_bits a widget can take: even, 2 .. most -- range_gate's own bound, and interval_gate's (interval_gate.hpp: 2^(num_bits + 1) < r)
constexpr uint64_t kRangeGateMaxBits = 254, kIntervalGateMaxBits = 252;
constexpr bool widget_num_bits_ok(uint64_t num_bits, uint64_t most) { return num_bits >= 2 && num_bits <= most && !(num_bits & 1); }
constexpr bool widget_shape_is(uint64_t num_bits, uint32_t k, uint32_t g, uint32_t pad) {
    return widget_shape(num_bits).k == k && widget_shape(num_bits).g == g && widget_shape(num_bits).pad == pad;
}
static_assert(widget_shape_is(2, 1, 1, 2), "one quad: no new Variable, P(0) .. P(2) are zero_var");
static_assert(widget_shape_is(6, 3, 1, 0), "a full row: no padding");
static_assert(widget_shape_is(8, 4, 2, 2), "the fourth quad opens a second row");
static_assert(widget_shape_is(254, 127, 43, 2) && widget_shape(254).rows() == 44, "the longest chain that cannot wrap");
static_assert(widget_num_bits_ok(2, 254) && widget_num_bits_ok(254, 254) && !widget_num_bits_ok(254, 252) && !widget_num_bits_ok(7, 254), "");

struct RangeGateArgs {
    const uint64_t *witness_vars;  // existing Variables
    const uint4 *witness;          // their assignments (gathered from the composer's table)
    uint32_t k, g, pad;            // quads, widget rows, leading positions that are zero_var beside P(0)
};

struct RangeGateGD {
    using Args = RangeGateArgs;
    struct alignas(16) ItemRec { Fr vc; };  // the witness's canonical integer: the accumulators are its prefixes
    static constexpr int W = 256;
    static constexpr int kInv = 0;
    __device__ static bool is_inv_slot(const Args &, const ItemRec &, uint32_t) { return false; }
    static constexpr bool kRagged = false, kRecInRows = false, kUsePow2 = false;
    __device__ static uint32_t rows_per_item(const Args &A) { return A.g + 1; }
    __device__ static uint32_t vars_per_item(const Args &A) { return A.k - 1; }
    __device__ static void fill_table(const Args &, uint4 *, uint32_t) {}
    __device__ static void item(const Args &A, const EmitOut &, uint64_t item, const uint4 *, ItemRec &R) {
        FrVec t;
        t.v[0] = A.witness[2 * item];
        t.v[1] = A.witness[2 * item + 1];
        R.vc = fr_from_mont(t.f);
    }
    __device__ static void selectors(const Args &, const ItemRec &, uint32_t, const uint4 *table, uint32_t h, uint4 out[5]) {
#pragma unroll
        for (int c = 0; c < 5; c++) out[c] = table[2 * T_ZERO + h];
    }
    // the Variable at position p of the item (the record is not read: the rows are a function of the call alone)
    __device__ static uint64_t position(const Args &A, const EmitOut &O, uint64_t item, uint64_t vbase, uint32_t p) {
        if (p <= A.pad) return O.zero_var;
        if (p < 3 * A.g) return vbase + (p - A.pad - 1);
        return A.witness_vars[item];
    }
    __device__ static void wires(const Args &A, const EmitOut &O, const ItemRec &, uint64_t item, uint64_t vbase, uint32_t j,
                                 uint64_t out[3]) {
        out[0] = position(A, O, item, vbase, 3 * j);
        out[1] = j < A.g ? position(A, O, item, vbase, 3 * j + 1) : O.zero_var;
        out[2] = j < A.g ? position(A, O, item, vbase, 3 * j + 2) : O.zero_var;
    }
    // new Variable kk sits at position pad + 1 + kk: the quads above it shifted away
    __device__ static Fr var_value(const Args &A, const ItemRec &R, const uint4 *, uint32_t kk) {
        return fr_to_mont(raw_shr(R.vc, 2 * (A.k - 1 - kk)));
    }
};

// the widget rows of the composer, merged when adjacent and alike
struct RangeSeg {
    uint64_t first, items;  // first row; items of g + 1 rows each
    uint32_t g;
};

// q_range = 1 on rows 0 .. g - 1 of every item of the segment (the column holds 0 there already): 16 bytes per lane
__global__ __launch_bounds__(kThreads) void range_patch_kernel(uint4 *q_range, const RangeSeg S) {
    FrVec one;
    one.f = fr_one();
    const uint64_t units = 2 * S.items * S.g;
    for (uint64_t u = (uint64_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += (uint64_t)gridDim.x * kThreads) {
        const uint64_t r = u >> 1, item = r / S.g, row = S.first + item * (S.g + 1) + (r - item * S.g);
        store16(q_range + 2 * row + (u & 1), (u & 1) ? one.v[1] : one.v[0]);
    }
}

// f in {0, 1, 2, 3}
__device__ __forceinline__ bool range_quad(const Fr &f) {
    const Fr c = fr_from_mont(f);
    return (c.l[1] | c.l[2] | c.l[3]) == 0 && c.l[0] < 4;
}

// the statement of every q_range = 1 row of the segment, from the wires and the assignments as they are in the columns; a wire
// that is no Variable of the composer marks the row as bad instead of being dereferenced.  First failing row -> *first_bad.
__global__ __launch_bounds__(kThreads) void range_check_rows_kernel(const ComposerCols C, const RangeSeg S, uint64_t n_vars,
                                                                    unsigned long long *first_bad) {
    const uint64_t rows = S.items * S.g;
    for (uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * kThreads) {
        const uint64_t item = r / S.g, row = S.first + item * (S.g + 1) + (r - item * S.g);
        const uint64_t w[4] = {C.w[0][row], C.w[1][row], C.w[2][row], C.w[0][row + 1]};
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; k++) ok = ok && w[k] < n_vars;
        if (ok) {
            FrVec v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                v[k].v[0] = C.vars[2 * w[k]];
                v[k].v[1] = C.vars[2 * w[k] + 1];
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const Fr twice = fr_add(v[k].f, v[k].f);
                ok = ok && range_quad(fr_sub(v[k + 1].f, fr_add(twice, twice)));
            }
        }
        if (!ok) atomicMin(first_bad, (unsigned long long)row);
    }
}

}  // namespace pg
