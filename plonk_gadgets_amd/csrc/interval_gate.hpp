// interval_gate.hpp -- interval_gate(witness, min, max, num_bits): min <= witness <= max with PUBLIC bounds, as two range widgets
// (range_gate.hpp) on the differences d_lo = witness - min and d_hi = max - witness: the gadget descriptor
// for the streaming writer (emit.hpp), with one (min, max) for the call or a pair per item, and the kernel that validates per-item
// bounds.
//
// num_bits even, 2 <= num_bits <= 252 (2^(num_bits + 1) < r), lo <= hi and hi - lo < 2^num_bits as canonical integers.  k, g and pad
// as in range_gate.hpp.  An item owns 2 (g + 1) rows and 2 k new Variables, in two halves h = 0 (d = witness - min) and h = 1
// (d = max - witness), half h in rows h (g + 1) .. and Variables first + h k ..:
//   Variable first + h k + kk = c(d) >> 2 (k - 1 - kk), kk = 0 .. k - 1, c(d) the canonical integer of d: the widget's k - 1
//   accumulators, then (shift 0) d itself
//   P(p) = zero_var (p <= pad);  first + h k + (p - pad - 1) (pad < p <= 3g): P(3g) is d
//   row i < g: (P(3i), P(3i+1), P(3i+2)), every arithmetic selector 0, q_range = 1 (a RangeSeg of 2 x batch items of g + 1 rows)
//   row g:     (d, witness, zero_var) with q_l = 1 and  q_r = -1, q_c = +min  (d - w + min = 0)   h = 0
//                                                      q_r = +1, q_c = -max  (d + w - max = 0)   h = 1
// The terminal row, vacuous in range_gate, carries the link between d and the witness: the subtraction costs no row.
// Soundness: both widgets hold => d_lo, d_hi in [0, 2^num_bits) and d_lo + d_hi = hi - lo (mod r); the left side is below
// 2^(num_bits + 1) < r and so is the right, hence equal as integers: d_lo <= hi - lo and witness = lo + d_lo in [lo, hi] without a
// wrap.  An out-of-range witness gets all its rows; the first accumulator of the failing half is >= 4, so that half's row 0 fails.
#pragma once

#include "composer.hpp"
#include "range_gate.hpp"

namespace pg {

struct IntervalGateArgs {
    const uint64_t *witness_vars;  // existing Variables
    const uint4 *witness;          // their assignments (gathered from the composer's table)
    Fr min, max;                   // one pair for the call (Montgomery form); not read when the bounds are per item
    const uint4 *min_v, *max_v;    // a pair per item (Montgomery form); not read otherwise
    uint32_t k, g, pad;            // quads, widget rows of a half, leading positions that are zero_var beside P(0)
};

template <bool PER_ITEM>
struct IntervalGateGD {
    using Args = IntervalGateArgs;
    struct alignas(16) RecUniform { Fr dc[2]; };         // canonical integers of witness - min, max - witness
    struct alignas(16) RecPerItem { Fr dc[2], qc[2]; };  // ... and q_c of the two terminal rows: mont(min), mont(-max) of this item
    using ItemRec = std::conditional_t<PER_ITEM, RecPerItem, RecUniform>;
    static constexpr int W = 256;
    static constexpr int kInv = 0;
    __device__ static bool is_inv_slot(const Args &, const ItemRec &, uint32_t) { return false; }
    static constexpr bool kRagged = false, kRecInRows = PER_ITEM, kUsePow2 = false;
    __device__ static uint32_t rows_per_item(const Args &A) { return 2 * (A.g + 1); }
    __device__ static uint32_t vars_per_item(const Args &A) { return 2 * A.k; }
    __device__ static void fill_table(const Args &A, uint4 *table, uint32_t tid) {
        if (tid == T_QC_A || tid == T_QC_B) {  // (per item: the items' own, from their records)
            FrVec t;
            t.f = PER_ITEM ? fr_zero() : (tid == T_QC_A ? A.min : fr_neg(A.max));
            table[2 * tid] = t.v[0];
            table[2 * tid + 1] = t.v[1];
        }
    }
    __device__ static Fr bound(const Args &A, const uint4 *v, const Fr &uniform, uint64_t item) {
        if constexpr (PER_ITEM) {
            FrVec t;
            t.v[0] = v[2 * item];
            t.v[1] = v[2 * item + 1];
            return t.f;
        } else {
            return uniform;
        }
    }
    // what the rows read: q_c of the item's terminal rows, functions of its PUBLIC bounds alone
    __device__ static void item_rows(const Args &A, const EmitOut &, uint64_t item, const uint4 *, ItemRec &R) {
        if constexpr (PER_ITEM) {
            R.qc[0] = bound(A, A.min_v, A.min, item);
            R.qc[1] = fr_neg(bound(A, A.max_v, A.max, item));
        }
    }
    __device__ static void item(const Args &A, const EmitOut &, uint64_t item, const uint4 *, ItemRec &R) {
        FrVec x;
        x.v[0] = A.witness[2 * item];
        x.v[1] = A.witness[2 * item + 1];
        R.dc[0] = fr_from_mont(fr_sub(x.f, bound(A, A.min_v, A.min, item)));
        R.dc[1] = fr_from_mont(fr_sub(bound(A, A.max_v, A.max, item), x.f));
    }
    __device__ static void selectors(const Args &A, const ItemRec &R, uint32_t j, const uint4 *table, uint32_t h, uint4 out[5]) {
        const uint32_t half = j > A.g ? 1u : 0u;
        const bool link = j - half * (A.g + 1) == A.g;  // the half's terminal row
        const uint4 zero = table[2 * T_ZERO + h];
        out[0] = zero;
        out[1] = link ? table[2 * T_ONE + h] : zero;
        out[2] = link ? table[2 * (half ? T_ONE : T_NEG1) + h] : zero;
        out[3] = zero;
        if constexpr (PER_ITEM) out[4] = link ? reinterpret_cast<const uint4 *>(R.qc)[2 * half + h] : zero;
        else out[4] = link ? table[2 * (T_QC_A + half) + h] : zero;
    }
    // the Variable at position p <= 3g of a half whose Variables start at hbase
    __device__ static uint64_t position(const Args &A, const EmitOut &O, uint64_t hbase, uint32_t p) {
        return p <= A.pad ? O.zero_var : hbase + (p - A.pad - 1);
    }
    // (the record is not read: the wires are a function of the call alone)
    __device__ static void wires(const Args &A, const EmitOut &O, const ItemRec &, uint64_t item, uint64_t vbase, uint32_t j,
                                 uint64_t out[3]) {
        const uint32_t half = j > A.g ? 1u : 0u, jj = j - half * (A.g + 1);
        const uint64_t hbase = vbase + half * A.k;
        out[0] = position(A, O, hbase, 3 * jj);
        out[1] = jj < A.g ? position(A, O, hbase, 3 * jj + 1) : A.witness_vars[item];
        out[2] = jj < A.g ? position(A, O, hbase, 3 * jj + 2) : O.zero_var;
    }
    // new Variable kk of a half: the quads of d below it shifted away (the last one, shift 0, is d)
    __device__ static Fr var_value(const Args &A, const ItemRec &R, const uint4 *, uint32_t kk) {
        const uint32_t half = kk >= A.k ? 1u : 0u;
        return fr_to_mont(raw_shr(R.dc[half], 2 * (A.k - 1 - (kk - half * A.k))));
    }
};

// per-item bounds against the preconditions, as canonical integers: both below r, lo <= hi, hi - lo < 2^num_bits.  One lane per
// item at a time; out->call[kIntervalBadItems] += the items that violate one, out->call[kIntervalFirstBad] = min of the first such item
// (it starts at ~0).  The lane has the item's eight words in registers, so the same pass digests the two arrays for the call's
// signature (out->others, digest.hpp: the pairs as ONE array of eight words per item -- a bound moved, the two arrays swapped, or two
// items' bounds swapped, is another call to pg_composer_clear_witness).  Every wave ends in two atomics on the same two words, which
// the memory system serialises (about 12 ns each on MI355X): the grid is a few workgroups per CU that stride over the items, not one
// workgroup per 256 items -- 16 384 waves' atomics took 405 us at 2^20 items where the arrays' 64 MiB are read in 40
enum : int { kIntervalFirstBad = 0, kIntervalBadItems = 1 };  // Preflight::call
__global__ __launch_bounds__(kThreads) void interval_bounds_kernel(const uint4 *min_v, const uint4 *max_v, uint64_t batch, uint32_t num_bits,
                                                                   Preflight *out) {
    Digest h{0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < batch; i += (uint64_t)gridDim.x * kThreads) {
        FrVec lo, hi;
        lo.v[0] = min_v[2 * i];
        lo.v[1] = min_v[2 * i + 1];
        hi.v[0] = max_v[2 * i];
        hi.v[1] = max_v[2 * i + 1];
#pragma unroll
        for (int j = 0; j < 8; j++) h.add(j < 4 ? lo.f.l[j] : hi.f.l[j - 4], 8 * i + j, scalar_array_salt(0));
        bool bad = !fr_raw_is_reduced(lo.f) || !fr_raw_is_reduced(hi.f) || raw_less(fr_from_mont(hi.f), fr_from_mont(lo.f));
        // hi >= lo: the field difference is the integer one
        const Fr top = raw_shr(fr_from_mont(fr_sub(hi.f, lo.f)), num_bits);
        bad = bad || (top.l[0] | top.l[1] | top.l[2] | top.l[3]) != 0;
        if (bad) {
            atomicAdd(&out->call[kIntervalBadItems], 1ull);
            atomicMin(&out->call[kIntervalFirstBad], (unsigned long long)i);
        }
    }
    digest_flush(h, &out->others);
}

}  // namespace pg
