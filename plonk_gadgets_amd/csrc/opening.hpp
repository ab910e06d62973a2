// opening.hpp -- the prover's round 5 over the scalar field (gfx950): a weighted sum of columns and its division by a linear
// factor, the KZG opening witness.
//
// With f = sum_j mu_j p_j over n_cols columns of n coefficients and a point x, pg_poly_open writes the Ruffini quotient of f by
// (X - x) and the remainder f(x).  Let Q_i = sum_{k >= i} f_k x^(k - i) (Q_n = 0): then q_{i-1} = Q_i, the witness is
// W[i] = Q_{i+1} (i < n, so W[n - 1] = Q_n = 0) and f(x) = Q_0.  Q is a reverse linear scan with multiplier x, done in three
// passes over tiles of kOpenTile coefficients, none of which waits on another workgroup:
//   1. open_combine_kernel<true>: a tile per workgroup step; lane t forms f at points base + 256 k + t (coalesced loads of every
//      column, the next column's load issued before the current multiplication), stores f into the witness buffer and runs
//      Horner along its points (acc = acc x^256 + f).  acc x^t summed over the lanes in LDS is the tile's total
//      S_b = sum_{k in tile} f_k x^(k - base), which lane 0 writes to the engine's workspace.
//   2. open_carry_kernel, one workgroup: lane L takes `chunk` consecutive tiles, forms its chunk's total by Horner with x^kOpenTile,
//      a reverse scan across the lanes (multiplier (x^kOpenTile)^chunk) gives it the carry from above, and it walks down its
//      chunk replacing S_b by C_b = Q_(base of tile b + 1) (C_b = S_(b+1) + x^kOpenTile C_(b+1)).  The bottom value is f(x).
//   3. open_quotient_kernel: a tile per workgroup step; the tile's f goes through LDS (coalesced in, padded by 16 bytes per run so
//      the reads are conflict-free) so that lane t holds the contiguous run of kOpenRun points at base + kOpenRun t.  The run's
//      total, a reverse scan across the lanes with multiplier x^kOpenRun and the tile's carry C_b give the lane Q at the top of its
//      run; Horner down the run gives Q_{i+1} at every point i, which goes back through LDS to a coalesced store over f.
// Multiplications per coefficient: n_cols (fewer where mu_j = 1) + 1 in pass 1, 2 + 6 / kOpenRun in pass 3.
// open_combine_kernel<false> is the sum alone (pg_poly_combine).  No scratch memory; LDS: 8 KiB (passes 1 and 2), 68 KiB
// (pass 3: two workgroups per CU); 64-bit indices throughout (n up to 2^32).
#pragma once

#include "quotient.hpp"

namespace pg {

constexpr uint32_t kOpenMaxCols = 32;
constexpr uint32_t kOpenRun = 8;                                             // contiguous points per lane in pass 3
constexpr uint64_t kOpenTile = (uint64_t)kThreads * kOpenRun;                // 2048 points
constexpr uint32_t kOpenLdsUnits = 2 * (uint32_t)kOpenTile + (uint32_t)kOpenTile / kOpenRun;  // uint4 units: 68 KiB

struct OpenArgs {
    const uint4 *col[kOpenMaxCols];  // the columns (may repeat)
    Fr mu[kOpenMaxCols];             // their weights
    uint32_t n_cols;
    uint32_t one_mask;               // bit j: mu_j = 1 (an addition instead of a multiplication)
    uint64_t n, tiles;               // tiles = ceil(n / kOpenTile)
    uint64_t chunk;                  // tiles per lane of pass 2: ceil(tiles / 256)
    uint4 *f;                        // the output column: f, then the witness
    uint4 *tot;                      // workspace, `tiles` entries: tile totals S_b, then carries C_b
    uint4 *value;                    // f(x)
    Fr xpow2[12];                    // x^(2^b), b < 12: x^t for t < 256, x^256, the run's x^(kOpenRun 2^k), x^kOpenTile
    Fr chunk_pow[8];                 // (x^(kOpenTile chunk))^(2^k), k < 8
};
static_assert(kOpenTile == 2048 && kOpenRun == 8, "xpow2 indices below: x^256 = 2^8, x^kOpenRun = 2^3, x^kOpenTile = 2^11");

__device__ __forceinline__ void open_lds_put(uint4 *lds, uint32_t e, const Fr &f) {
    FrVec v;
    v.f = f;
    const uint32_t u = 2 * e + e / kOpenRun;
    lds[u] = v.v[0];
    lds[u + 1] = v.v[1];
}
__device__ __forceinline__ Fr open_lds_get(const uint4 *lds, uint32_t e) {
    FrVec v;
    const uint32_t u = 2 * e + e / kOpenRun;
    v.v[0] = lds[u];
    v.v[1] = lds[u + 1];
    return v.f;
}

// the reverse exclusive scan across the 256 lanes: sum_{t' > t} v_t' M^(t' - t - 1), pw[k] = M^(2^k); buf: 256 entries of LDS
__device__ __forceinline__ Fr open_lane_scan(const Fr &v, const Fr *pw, FrVec *buf) {
    const uint32_t t = threadIdx.x;
    Fr s = v;
#pragma unroll 1
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t d = 1u << k;
        buf[t].f = s;
        __syncthreads();
        if (t + d < kThreads) s = fr_add(s, fr_mul(pw[k], buf[t + d].f));
        __syncthreads();
    }
    buf[t].f = s;
    __syncthreads();
    const Fr r = t + 1 < kThreads ? buf[t + 1].f : fr_zero();
    __syncthreads();  // (buf is reused)
    return r;
}

// pass 1 (TOTALS) or the whole of pg_poly_combine
template <bool TOTALS>
__global__ __launch_bounds__(kThreads) void open_combine_kernel(const OpenArgs A) {
    __shared__ FrVec buf[TOTALS ? kThreads : 1];
    const uint32_t t = threadIdx.x;
    Fr xt = fr_one();  // x^t
    if (TOTALS) {
#pragma unroll 1
        for (uint32_t b = 0; b < 8; b++)
            if ((t >> b) & 1) xt = fr_mul(xt, A.xpow2[b]);
    }
#pragma unroll 1
    for (uint64_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const uint64_t base = tile * kOpenTile;
        Fr acc = fr_zero();
#pragma unroll 1
        for (int k = (int)kOpenRun - 1; k >= 0; k--) {
            const uint64_t i = base + (uint64_t)k * kThreads + t;
            Fr f = fr_zero();
            if (i < A.n) {
                Fr p = pp_load(A.col[0], i);
#pragma unroll 1
                for (uint32_t j = 0; j < A.n_cols; j++) {
                    const Fr next = j + 1 < A.n_cols ? pp_load(A.col[j + 1], i) : p;
                    f = fr_add(f, (A.one_mask >> j) & 1 ? p : fr_mul(A.mu[j], p));
                    p = next;
                }
                pp_store(A.f, i, f);
            }
            if (TOTALS) acc = fr_add(fr_mul(acc, A.xpow2[8]), f);
        }
        if (TOTALS) {
            const Fr s = eval_block_sum(fr_mul(acc, xt), buf);
            if (t == 0) pp_store(A.tot, tile, s);
        }
    }
}

// pass 2: one workgroup of kThreads lanes
__global__ __launch_bounds__(kThreads) void open_carry_kernel(const OpenArgs A) {
    __shared__ FrVec buf[kThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t first = (uint64_t)t * A.chunk;
    const Fr x_tile = A.xpow2[11];
    const uint64_t mine = first < A.tiles ? (A.tiles - first < A.chunk ? A.tiles - first : A.chunk) : 0;  // tiles of this lane
    // (each loop loads the next total before it multiplies: the chain of multiplications is the lane's critical path)
    Fr acc = fr_zero(), s = mine ? pp_load(A.tot, first + mine - 1) : fr_zero();
#pragma unroll 1
    for (uint64_t j = mine; j-- > 0;) {
        const Fr next = j ? pp_load(A.tot, first + j - 1) : s;
        acc = fr_add(fr_mul(acc, x_tile), s);
        s = next;
    }
    Fr c = open_lane_scan(acc, A.chunk_pow, buf);  // C of the lane's top tile (0 above the last tile)
    s = mine ? pp_load(A.tot, first + mine - 1) : fr_zero();
#pragma unroll 1
    for (uint64_t j = mine; j-- > 0;) {
        const Fr next = j ? pp_load(A.tot, first + j - 1) : s;
        pp_store(A.tot, first + j, c);
        c = fr_add(s, fr_mul(x_tile, c));
        s = next;
    }
    if (t == 0) pp_store(A.value, 0, c);  // Q_0 = f(x)
}

// pass 3
__global__ __launch_bounds__(kThreads) void open_quotient_kernel(const OpenArgs A) {
    __shared__ uint4 lds[kOpenLdsUnits];
    const uint32_t t = threadIdx.x;
    const Fr x = A.xpow2[0];
#pragma unroll 1
    for (uint64_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const uint64_t base = tile * kOpenTile;
#pragma unroll
        for (uint32_t k = 0; k < kOpenRun; k++) {
            const uint32_t e = k * kThreads + t;
            open_lds_put(lds, e, base + e < A.n ? pp_load(A.f, base + e) : fr_zero());
        }
        __syncthreads();
        Fr run[kOpenRun];
#pragma unroll
        for (uint32_t j = 0; j < kOpenRun; j++) run[j] = open_lds_get(lds, t * kOpenRun + j);
        __syncthreads();
        // the run's total sum_j run[j] x^j; lane 255 adds the tile's carry C_b one run above it
        Fr v = run[kOpenRun - 1];
#pragma unroll
        for (int j = (int)kOpenRun - 2; j >= 0; j--) v = fr_add(run[j], fr_mul(x, v));
        const Fr carry = pp_load(A.tot, tile);
        if (t == kThreads - 1) v = fr_add(v, fr_mul(A.xpow2[3], carry));
        Fr q = open_lane_scan(v, A.xpow2 + 3, reinterpret_cast<FrVec *>(lds));
        if (t == kThreads - 1) q = carry;  // Q one past the run's top
        // Horner down the run: the witness at point i is Q_{i+1}
#pragma unroll
        for (int j = (int)kOpenRun - 1; j >= 0; j--) {
            const Fr fj = run[j];
            run[j] = q;
            if (j) q = fr_add(fj, fr_mul(x, q));
        }
#pragma unroll
        for (uint32_t j = 0; j < kOpenRun; j++) open_lds_put(lds, t * kOpenRun + j, run[j]);
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kOpenRun; k++) {
            const uint32_t e = k * kThreads + t;
            if (base + e < A.n) pp_store(A.f, base + e, open_lds_get(lds, e));
        }
        __syncthreads();
    }
}

}  // namespace pg
