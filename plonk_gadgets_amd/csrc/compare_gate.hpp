// compare_gate.hpp -- is_less_equal(x, y, num_bits, strict): the bit [x <= y] (strict: [x < y]) of two WITNESSES as a Variable, from
// ONE range widget (range_gate.hpp) on z = 2^num_bits + y - x - s, s = 1 if strict else 0: the gadget
// descriptor for the streaming writer (emit.hpp).
//
// num_bits even, 2 <= num_bits <= 252 (2^(num_bits + 1) < r).  K = num_bits + 2, k = K / 2 quads, g = ceil(k / 3) widget rows,
// pad = 3g - k: the shape of a range widget over K bits.  c(z) is the canonical integer of z.  An item owns g + 1 rows and k new
// Variables first + kk, kk = 0 .. k - 1:
//   Variable first + kk = c(z) >> 2 (k - 1 - kk): the widget's k - 1 accumulators, then (shift 0) z itself.  first holds the TOP
//   quad of c(z), bits num_bits and num_bits + 1: it is the RESULT
//   P(p) = zero_var (p <= pad);  first + (p - pad - 1) (pad < p <= 3g): P(3g) is z
//   row i < g: (P(3i), P(3i+1), P(3i+2)), every arithmetic selector 0, q_range = 1 (a RangeSeg of batch items of g + 1 rows)
//   row g:     (z, y, x) with q_l = 1, q_r = -1, q_o = +1, q_c = -2^num_bits + s   (z - y + x - 2^num_bits + s = 0)
// The terminal row, vacuous in range_gate, links z to the two witnesses: the comparison costs no row beyond the widget's.
//
// What it proves.  PRECONDITION: the circuit bounds x and y below 2^num_bits (range_gate or interval_gate at <= num_bits bits on
// each).  Then 1 - s <= 2^num_bits + y - x - s < 2^(num_bits + 1) < r: no wrap, c(z) is that integer, its quad at bit position
// num_bits is 0 or 1, and it is 1 exactly when y - x - s >= 0: result = [x <= y], or [x < y] when strict.  WITHOUT the precondition
// the rows state c(z) < 2^K alone and the result is a quad without meaning (x = r - 1, y = 0: z = 2^num_bits + 1, result 1).  The
// gadget adds no boolean row and does not bound its inputs: that is the circuit author's part, as interval_gate's preconditions
// are.  An item whose c(z) >= 2^K (x = 0, y = 3 * 2^num_bits) still gets all its rows; its first accumulator is >= 4, so the
// item's row 0 fails.
#pragma once

#include "range_gate.hpp"

namespace pg {

constexpr uint64_t kCompareGateMaxBits = 252;
// the widget's shape for a comparison at num_bits: a range widget over num_bits + 2 bits
constexpr WidgetShape compare_shape(uint64_t num_bits) { return widget_shape(num_bits + 2); }
static_assert(compare_shape(2).k == 2 && compare_shape(2).g == 1 && compare_shape(2).pad == 1, "");
static_assert(compare_shape(64).k == 33 && compare_shape(64).rows() == 12, "64 bits: 12 rows, 33 Variables");
static_assert(compare_shape(252).k == 127 && compare_shape(252).pad == 2, "the widest: range_gate's longest chain");

struct CompareGateArgs {
    const uint64_t *x_vars, *y_vars;  // existing Variables
    const uint4 *x, *y;               // their assignments (gathered from the composer's table)
    Fr offset;                        // mont(2^num_bits - s); q_c of the terminal row is its negative
    uint64_t *result_vars;            // [batch]: the item's first new Variable (may be NULL)
    uint32_t k, g, pad;               // quads, widget rows, leading positions that are zero_var beside P(0)
};

struct CompareGateGD {
    using Args = CompareGateArgs;
    struct alignas(16) ItemRec { Fr zc; };  // c(z): the new Variables are its prefixes
    static constexpr int W = 256;
    static constexpr int kInv = 0;
    __device__ static bool is_inv_slot(const Args &, const ItemRec &, uint32_t) { return false; }
    static constexpr bool kRagged = false, kRecInRows = false, kUsePow2 = false;
    __device__ static uint32_t rows_per_item(const Args &A) { return A.g + 1; }
    __device__ static uint32_t vars_per_item(const Args &A) { return A.k; }
    __device__ static void fill_table(const Args &A, uint4 *table, uint32_t tid) {
        if (tid == T_QC_A || tid == T_QC_B) {  // (T_QC_B is not read: filled so that no slot of the table is left as it was)
            FrVec t;
            t.f = tid == T_QC_A ? fr_neg(A.offset) : fr_zero();
            table[2 * tid] = t.v[0];
            table[2 * tid + 1] = t.v[1];
        }
    }
    __device__ static void item(const Args &A, const EmitOut &O, uint64_t item, const uint4 *, ItemRec &R) {
        FrVec x, y;
        x.v[0] = A.x[2 * item];
        x.v[1] = A.x[2 * item + 1];
        y.v[0] = A.y[2 * item];
        y.v[1] = A.y[2 * item + 1];
        R.zc = fr_from_mont(fr_sub(fr_add(A.offset, y.f), x.f));
        if (A.result_vars) A.result_vars[item] = O.var_base + item * A.k;
    }
    __device__ static void selectors(const Args &A, const ItemRec &, uint32_t j, const uint4 *table, uint32_t h, uint4 out[5]) {
        const bool link = j == A.g;  // the terminal row
        const uint4 zero = table[2 * T_ZERO + h], one = table[2 * T_ONE + h];
        out[0] = zero;
        out[1] = link ? one : zero;
        out[2] = link ? table[2 * T_NEG1 + h] : zero;
        out[3] = link ? one : zero;
        out[4] = link ? table[2 * T_QC_A + h] : zero;
    }
    // the Variable at position p <= 3g of the item
    __device__ static uint64_t position(const Args &A, const EmitOut &O, uint64_t vbase, uint32_t p) {
        return p <= A.pad ? O.zero_var : vbase + (p - A.pad - 1);
    }
    // (the record is not read: the wires are a function of the call alone)
    __device__ static void wires(const Args &A, const EmitOut &O, const ItemRec &, uint64_t item, uint64_t vbase, uint32_t j,
                                 uint64_t out[3]) {
        out[0] = position(A, O, vbase, 3 * j);
        out[1] = j < A.g ? position(A, O, vbase, 3 * j + 1) : A.y_vars[item];
        out[2] = j < A.g ? position(A, O, vbase, 3 * j + 2) : A.x_vars[item];
    }
    // new Variable kk: the quads of c(z) below it shifted away (the last one, shift 0, is z)
    __device__ static Fr var_value(const Args &A, const ItemRec &R, const uint4 *, uint32_t kk) {
        return fr_to_mont(raw_shr(R.zc, 2 * (A.k - 1 - kk)));
    }
};

}  // namespace pg
