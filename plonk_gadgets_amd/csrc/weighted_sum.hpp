// weighted_sum.hpp -- weighted_sum_ragged_batch: result[s] = k[s] + sum over the terms t of segment s of
// c[t] * value(x[t]), as the chain of composer.add calls a user of the reference would write:
//   acc = add((c[b], x[b]), (c[b+1], x[b+1]), k[s]);  for t = b+2 .. e: acc = add((1, acc), (c[t], x[t]), 0)
// Segment s has the terms b = seg_off[s] .. e = seg_off[s+1] - 1, at least two.  Term t with b < t <= e owns row (and new Variable)
// t - s - 1 of the call; a segment's first term owns neither:
//   t = b+1:  wires (x[b], x[b+1], new)        q_l = c[b]  q_r = c[b+1]  q_o = -1  q_c = k[s]
//   t > b+1:  wires (new - 1, x[t], new)       q_l = 1     q_r = c[t]    q_o = -1  q_c = 0
// and the new Variable holds k[s] + sum_{i = b .. t} c[i] value(x[i]): a segmented inclusive prefix sum over the scalar field.
//
// Parallel over TERMS: a tile is kWsTile consecutive terms, whatever segments they belong to; a lane owns kWsTermsPerLane consecutive
// terms of it.  Inside a tile the scan is segmented (it restarts where a segment starts); what a tile hands to the next -- the sum
// since its last segment start, and whether it has one -- goes through separate launches, as the grand product's (section 3.8):
//   1. weighted_sum_tiles_kernel   a tile per workgroup: its aggregate
//   2. weighted_sum_carry_kernel   ONE workgroup: the segmented exclusive scan of the aggregates, kWsCarryPass tiles at a time
//   3. weighted_sum_write_kernel   a tile per workgroup: the scan again, plus the tile's carry, then the tile's rows -- contiguous
//                                  in every column -- from LDS, 16 bytes per lane; <false>: var_values alone (a witness refresh)
// No workgroup waits for another inside a launch.  A call of one tile needs no carry: launch 3 alone.
// A term's segment: the tile's first segment by bisection of seg_off, then a count of starts carried through the same scan.  The
// kernels index with seg_off: the composer validates it (weighted_sum_check_kernel) before any of them runs.
#pragma once

#include "composer.hpp"
#include "emit.hpp"

namespace pg {

constexpr uint32_t kWsTermsPerLane = 4;
constexpr uint32_t kWsTile = kThreads * kWsTermsPerLane;  // terms per workgroup step (pg_weighted_sum_geometry)
constexpr uint32_t kWsCarryPass = kThreads;               // tile aggregates the carry launch scans at a time (one per lane)
constexpr uint32_t kWsStartsPerTile = kWsTile / 2 + 1;    // entries of seg_off in [base, base + kWsTile]: segments have >= 2 terms
static_assert((kWsTile & (kWsTile - 1)) == 0 && kWsTile < (1u << 15), "rowterm packs a term's place in 15 bits");

struct WeightedSumArgs {
    const uint64_t *term_var;  // [terms] existing Variables
    const uint64_t *seg_off;   // [segments + 1], validated
    const uint4 *val;          // [terms] their assignments (gathered from the composer's table)
    const uint4 *coeff;        // [terms] or NULL: all 1
    const uint4 *konst;        // [segments] or NULL: all 0
    uint64_t terms, segments, tiles;
    uint4 *tile_sum;           // [tiles] the sum since the tile's last segment start (the whole tile's where it has none)
    uint32_t *tile_flag;       // [tiles] it has one
    uint4 *tile_carry;         // [tiles] what the terms before the tile's first start add; NULL: one tile, nothing
    uint4 *q[5];               // the call's first row in the five selector columns
    uint64_t *w[3];            // ... and in the three wire columns
    uint4 *vars;               // the call's first new Variable in the table
    uint64_t var_base;         // its number
    uint64_t *result_vars;     // [segments] or NULL
};

// An element of the segmented scan is a sum and a word `meta`: bit 31 = a segment starts inside; below it, how many do.  (Kept as
// two values, not a struct: a struct of them that crosses a loop went to private memory.)
constexpr uint32_t kWsStart = 0x80000000u;
// (a, then b) -> b
__device__ __forceinline__ void ws_combine(const Fr &a_sum, uint32_t a_meta, Fr &b_sum, uint32_t &b_meta) {
    if (!(b_meta & kWsStart)) b_sum = fr_add(a_sum, b_sum);
    b_meta = ((a_meta | b_meta) & kWsStart) | ((a_meta + b_meta) & ~kWsStart);
}

// 256 lanes' elements -> what the lanes before lane t combine to (`before`; the identity for lane 0) and all 256 (`total`).
// sum: 2 x 256 entries of LDS, meta likewise.  Every lane of the workgroup calls it; the buffers are free when it returns.
__device__ __forceinline__ void ws_block_scan(Fr v_sum, uint32_t v_meta, FrVec *sum, uint32_t *meta, Fr &before_sum, uint32_t &before_meta,
                                              Fr &total_sum, uint32_t &total_meta) {
    const uint32_t t = threadIdx.x;
    uint32_t cur = 0;
    sum[t].f = v_sum;
    meta[t] = v_meta;
    __syncthreads();
#pragma unroll 1
    for (uint32_t off = 1; off < kThreads; off <<= 1) {
        if (t >= off) ws_combine(sum[cur + t - off].f, meta[cur + t - off], v_sum, v_meta);
        cur ^= kThreads;
        sum[cur + t].f = v_sum;
        meta[cur + t] = v_meta;
        __syncthreads();
    }
    before_sum = t ? sum[cur + t - 1].f : fr_zero();
    before_meta = t ? meta[cur + t - 1] : 0u;
    total_sum = sum[cur + kThreads - 1].f;
    total_meta = meta[cur + kThreads - 1];
    __syncthreads();
}

__device__ __forceinline__ Fr ws_load(const uint4 *a, uint64_t i) {
    FrVec t;
    t.v[0] = a[2 * i];
    t.v[1] = a[2 * i + 1];
    return t.f;
}

// the first j in [0, segments] with seg_off[j] >= t (t < terms = seg_off[segments]).  The same for every lane of the workgroup
__device__ __forceinline__ uint64_t ws_lower_bound(const uint64_t *seg_off, uint64_t segments, uint64_t t) {
    uint64_t lo = 0, hi = segments;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (seg_off[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// What a lane knows of its kWsTermsPerLane terms after the tile's scan.  Named members, no arrays: nothing here is indexed by a
// variable
struct WsLane {
    Fr p0, p1, p2, p3;  // the segmented inclusive sums inside the TILE at the lane's terms (the carry of the tile is not in them)
    uint32_t starts;    // bit i: term i starts a segment
    Fr before_sum;      // the lanes before this one
    uint32_t before_meta, total_meta;  // ... and the whole tile (its sum is a value of its own: ws_tile_scan)
    uint64_t lo;        // the first segment that starts at or behind the tile's first term
};

// p = c[t] * value(x[t]) (+ k[s] where t starts segment s); 0 beyond the call's last term
__device__ __forceinline__ Fr ws_term(const WeightedSumArgs &A, const uint16_t *start, uint64_t base, uint64_t lo, uint64_t t, uint32_t bit,
                                      uint32_t &starts) {
    if (t >= A.terms) return fr_zero();
    Fr p = ws_load(A.val, t);
    if (A.coeff) p = fr_mul(ws_load(A.coeff, t), p);
    const uint32_t s16 = start[t - base];
    if (s16) {
        starts |= bit;
        if (A.konst) p = fr_add(p, ws_load(A.konst, lo + s16 - 1));
    }
    return p;
}

// The scan of tile `tile`.  start: kWsTile entries of LDS, left filled: start[x] = 0, or 1 + (s - lo) where segment s starts at
// term base + x.  RESULTS: result_vars[s] for every segment that ENDS inside (base, base + kWsTile]
template <bool RESULTS>
__device__ __forceinline__ void ws_tile_scan(const WeightedSumArgs &A, uint64_t tile, FrVec *sum, uint32_t *meta, uint16_t *start, WsLane &L,
                                             Fr &total_sum) {
    const uint32_t tid = threadIdx.x;
    const uint64_t base = tile * kWsTile;
    L.lo = ws_lower_bound(A.seg_off, A.segments, base);
    for (uint32_t x = tid; x < kWsTile; x += kThreads) start[x] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < kWsStartsPerTile; i += kThreads) {
        const uint64_t j = L.lo + i;
        if (j > A.segments) break;
        const uint64_t o = A.seg_off[j];  // >= base
        if (o > base + kWsTile) break;
        if (j < A.segments && o < base + kWsTile) start[o - base] = (uint16_t)(1 + i);
        if (RESULTS && A.result_vars && j >= 1 && o > base) A.result_vars[j - 1] = A.var_base + o - j - 1;
    }
    __syncthreads();
    const uint64_t t0 = base + (uint64_t)tid * kWsTermsPerLane;
    L.starts = 0;
    L.p0 = ws_term(A, start, base, L.lo, t0, 1u, L.starts);
    L.p1 = ws_term(A, start, base, L.lo, t0 + 1, 2u, L.starts);
    L.p2 = ws_term(A, start, base, L.lo, t0 + 2, 4u, L.starts);
    L.p3 = ws_term(A, start, base, L.lo, t0 + 3, 8u, L.starts);
    if (!(L.starts & 2u)) L.p1 = fr_add(L.p0, L.p1);
    if (!(L.starts & 4u)) L.p2 = fr_add(L.p1, L.p2);
    if (!(L.starts & 8u)) L.p3 = fr_add(L.p2, L.p3);
    ws_block_scan(L.p3, (L.starts ? kWsStart : 0u) | (uint32_t)__popc(L.starts), sum, meta, L.before_sum, L.before_meta, total_sum,
                  L.total_meta);
    // what the lanes before add reaches the lane's terms up to its own first start
    if (!(L.starts & 1u)) L.p0 = fr_add(L.before_sum, L.p0);
    if (!(L.starts & 3u)) L.p1 = fr_add(L.before_sum, L.p1);
    if (!(L.starts & 7u)) L.p2 = fr_add(L.before_sum, L.p2);
    if (!(L.starts & 15u)) L.p3 = fr_add(L.before_sum, L.p3);
}

// launch 1: a tile per workgroup
__global__ __launch_bounds__(kThreads) void weighted_sum_tiles_kernel(const WeightedSumArgs A) {
    __shared__ uint4 s_sum[4 * kThreads];
    __shared__ uint32_t s_meta[2 * kThreads];
    __shared__ uint16_t s_start[kWsTile];
    WsLane L;
    Fr total;
    ws_tile_scan<false>(A, blockIdx.x, reinterpret_cast<FrVec *>(s_sum), s_meta, s_start, L, total);
    if (threadIdx.x == 0) {
        // (limb by limb: the total comes straight from LDS, and repacking it through a FrVec went through private memory)
        uint64_t *dst = reinterpret_cast<uint64_t *>(A.tile_sum + 2 * (uint64_t)blockIdx.x);
        dst[0] = total.l[0];
        dst[1] = total.l[1];
        dst[2] = total.l[2];
        dst[3] = total.l[3];
        A.tile_flag[blockIdx.x] = L.total_meta >> 31;
    }
}

// launch 2: one workgroup
__global__ __launch_bounds__(kThreads) void weighted_sum_carry_kernel(const WeightedSumArgs A) {
    __shared__ FrVec s_sum[2 * kThreads];
    __shared__ uint32_t s_meta[2 * kThreads];
    Fr running = fr_zero();  // the sum since the last start before the pass
#pragma unroll 1
    for (uint64_t first = 0; first < A.tiles; first += kWsCarryPass) {
        const uint64_t i = first + threadIdx.x;
        Fr before_sum, total_sum;
        uint32_t before_meta, total_meta;
        ws_block_scan(i < A.tiles ? ws_load(A.tile_sum, i) : fr_zero(), i < A.tiles && A.tile_flag[i] ? kWsStart : 0u, s_sum, s_meta,
                      before_sum, before_meta, total_sum, total_meta);
        if (i < A.tiles) {
            FrVec c;
            c.f = before_sum;
            if (!(before_meta & kWsStart)) c.f = fr_add(running, before_sum);
            A.tile_carry[2 * i] = c.v[0];
            A.tile_carry[2 * i + 1] = c.v[1];
        }
        running = (total_meta & kWsStart) ? total_sum : fr_add(running, total_sum);
    }
}

// launch 3: a tile per workgroup
template <bool FULL>
__global__ __launch_bounds__(kThreads) void weighted_sum_write_kernel(const WeightedSumArgs A) {
    __shared__ uint4 s_vals[2 * kWsTile];  // the tile's new assignments by row; before that, the scan's sums
    __shared__ uint32_t s_meta[2 * kThreads];
    __shared__ uint16_t s_start[kWsTile];
    __shared__ uint16_t s_rowterm[kWsTile];  // by row: the term that owns it (its place in the tile); bit 15: the segment's first row
    static_assert(sizeof(FrVec) * 2 * kThreads <= sizeof(uint4) * 2 * kWsTile, "the scan's sums fit where the assignments go");
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = blockIdx.x, base = tile * kWsTile;
    WsLane L;
    Fr total;  // (not used: the tile's carry comes from launch 2)
    ws_tile_scan<true>(A, tile, reinterpret_cast<FrVec *>(s_vals), s_meta, s_start, L, total);
    const Fr carry = A.tile_carry ? ws_load(A.tile_carry, tile) : fr_zero();
    // is the term before the tile a segment's first?  (then the tile's first term is no start, and its segment is lo - 1)
    const bool prev_start = base > 0 && L.lo > 0 && A.seg_off[L.lo - 1] == base - 1;
    const bool open = !(L.before_meta & kWsStart);  // no start in the tile before this lane
    const uint32_t cnt = L.before_meta & ~kWsStart;
    const uint32_t x0 = tid * kWsTermsPerLane;
    auto place = [&](const Fr &p, uint32_t i) {
        const uint32_t x = x0 + i, upto = L.starts & ((2u << i) - 1u);
        if (base + x >= A.terms || (L.starts >> i & 1u)) return;
        const uint32_t r = x - (cnt + (uint32_t)__popc(upto));
        FrVec v;
        v.f = open && !upto ? fr_add(carry, p) : p;
        s_vals[2 * r] = v.v[0];
        s_vals[2 * r + 1] = v.v[1];
        const bool first = x ? s_start[x - 1] != 0 : prev_start;
        s_rowterm[r] = (uint16_t)(x | (first ? 0x8000u : 0u));
    };
    place(L.p0, 0);
    place(L.p1, 1);
    place(L.p2, 2);
    place(L.p3, 3);
    __syncthreads();
    const uint64_t in_tile = A.terms - base < kWsTile ? A.terms - base : kWsTile;
    const uint32_t nrows = (uint32_t)in_tile - (L.total_meta & ~kWsStart);
    const uint64_t row0 = base - L.lo;  // the tile's first row, counted from the call's: term t of segment s owns row t - s - 1
    for (uint32_t u = tid; u < 2 * nrows; u += kThreads) store16(A.vars + 2 * row0 + u, s_vals[u]);
    if constexpr (FULL) {
        FrVec one, neg1;
        one.f = fr_one();
        neg1.f = fr_neg_one();
        const uint4 zero = make_uint4(0, 0, 0, 0);
        for (uint32_t u = tid; u < 2 * nrows; u += kThreads) {
            const uint32_t r = u >> 1, h = u & 1u, rt = s_rowterm[r];
            const bool first = rt >> 15;
            const uint64_t t = base + (rt & 0x7fffu), s = t - 1 - (row0 + r);
            const uint4 one_h = h ? one.v[1] : one.v[0];
            const uint4 q_l = first && A.coeff ? A.coeff[2 * (t - 1) + h] : one_h;
            const uint4 q_r = A.coeff ? A.coeff[2 * t + h] : one_h;
            const uint4 q_c = first && A.konst ? A.konst[2 * s + h] : zero;
            const uint64_t g = 2 * row0 + u;
            store16(A.q[0] + g, zero);
            store16(A.q[1] + g, q_l);
            store16(A.q[2] + g, q_r);
            store16(A.q[3] + g, h ? neg1.v[1] : neg1.v[0]);
            store16(A.q[4] + g, q_c);
        }
        // the wires: two rows' to a lane, from the first 16-byte boundary at or before the tile's first row
#pragma unroll
        for (int k = 0; k < 3; k++) {
            uint64_t *col = A.w[k] + row0;
            auto wire = [&](uint32_t r) -> uint64_t {
                const uint32_t rt = s_rowterm[r];
                const uint64_t t = base + (rt & 0x7fffu), fresh = A.var_base + row0 + r;
                if (k == 2) return fresh;
                if (k == 1) return A.term_var[t];
                return (rt >> 15) ? A.term_var[t - 1] : fresh - 1;
            };
            const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(col) >> 3) & 1u;
            for (uint32_t pr = tid; 2 * pr < nrows + mis; pr += kThreads) {
                const int64_t r0 = 2 * (int64_t)pr - mis, r1 = r0 + 1;
                const bool have0 = r0 >= 0, have1 = r1 < (int64_t)nrows;
                const uint64_t w0 = have0 ? wire((uint32_t)r0) : 0, w1 = have1 ? wire((uint32_t)r1) : 0;
                if (have0 && have1)
                    store16(reinterpret_cast<uint4 *>(col + r0),
                            make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)));
                else if (have0) col[r0] = w0;
                else if (have1) col[r1] = w1;
            }
        }
    }
}

// The call's other device arrays against its preconditions, and their digest, in one launch:
//   seg_off[0] == 0, seg_off[segments] == terms, every segment >= 2 terms     first offender -> out->call[kWsBadSegment]
//   every coefficient (coeff != NULL) below r                                 -> out->call[kWsBadCoeff]
//   every constant (konst != NULL) below r                                    -> out->call[kWsBadConstant]
//   (atomicMin; each starts at ~0)
//   out->others += every word of the three arrays, each array under its own salt (digest.hpp)
// A grid of a few workgroups per CU that stride over the entries: every wave ends in two atomics on the same words
// (interval_gate.hpp says what 16 384 waves' cost).
enum : int { kWsBadSegment = 0, kWsBadCoeff = 1, kWsBadConstant = 2 };  // Preflight::call
__global__ __launch_bounds__(kThreads) void weighted_sum_check_kernel(const uint64_t *seg_off, const uint4 *coeff, const uint4 *konst,
                                                                      uint64_t terms, uint64_t segments, Preflight *out) {
    Digest h{0, 0};
    const uint64_t lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x, stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t s = lane; s < segments; s += stride) {
        const uint64_t a = seg_off[s], b = seg_off[s + 1];
        if (s == 0) h.add(a, 0, kSaltSegOff);
        h.add(b, s + 1, kSaltSegOff);
        const bool bad = (s == 0 && a != 0) || b < a || b - a < 2 || (s == segments - 1 && b != terms);
        if (bad) atomicMin(&out->call[kWsBadSegment], (unsigned long long)s);
    }
    if (coeff)
        for (uint64_t t = lane; t < terms; t += stride) {
            const Fr x = ws_load(coeff, t);
#pragma unroll
            for (int j = 0; j < 4; j++) h.add(x.l[j], 4 * t + j, kSaltCoeff);
            if (!fr_raw_is_reduced(x)) atomicMin(&out->call[kWsBadCoeff], (unsigned long long)t);
        }
    if (konst)
        for (uint64_t s = lane; s < segments; s += stride) {
            const Fr x = ws_load(konst, s);
#pragma unroll
            for (int j = 0; j < 4; j++) h.add(x.l[j], 4 * s + j, kSaltConstant);
            if (!fr_raw_is_reduced(x)) atomicMin(&out->call[kWsBadConstant], (unsigned long long)s);
        }
    digest_flush(h, &out->others);
}

}  // namespace pg
