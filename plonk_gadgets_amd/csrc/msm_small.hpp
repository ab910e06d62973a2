// msm_small.hpp -- many small sums over BLS12-381 G1 in one pass (gfx950): the kernels of pg_msm_segmented (DESIGN section
// 3.15).  msm.hpp's Pippenger pays 16 sorts and 2^15 buckets per window whatever n is; a verifier wants thousands of sums of
// ~27 points each.  Here every product s_j[i] P_i is a fixed-window scalar multiplication on a lane of its own, and every
// (segment, column) is then summed by one wave.
//
//   * msm_seg_mul_kernel<W>: lane t = j n + i computes s_j[i] P_i.  The scalar leaves Montgomery form as in msm_digits_kernel and
//     is cut into kWindows = floor(255 / W) + 1 signed digits of W bits: window k's raw value r (its W bits plus the carry of
//     window k - 1) is the digit r when r <= 2^(W-1), else r - 2^W with a carry into window k + 1.  A scalar is < r_Fr < 2^255,
//     so the top window holds at most W - 1 of its bits (W = 4: bits 252..254; W = 3: none, it starts at bit 255) and its raw
//     value is at most 2^(W-1) - 1 + 1: the carry out of the last window is always 0 and kWindows windows cover every scalar.
//     |digit| is in [0, 2^(W-1)]: the lane keeps 2 P .. 2^(W-1) P (XYZZ, 192 bytes each) in LDS, word k of lane l at
//     [slot][k][l] (a 64-bit access of a wave then touches every bank once, whichever slot each lane picks), and reads P itself
//     back from the bases.  From the top window down: W doublings, then one g1x_add of +- the digit's multiple (none for a
//     digit 0): every lane of a wave runs the same kWindows steps, whatever its scalar.  The carries are found first, from the
//     bottom up, and kept as a bit mask (the digits are needed from the top down).
//     Every addition is g1.hpp's complete g1x_add: the accumulator meets +- a table entry for small scalars (2 P + 2 P ...),
//     the identity for identity bases and zero scalars.
//   * msm_seg_sum_kernel: one wave per (segment, column).  Lane l adds the products l, l + 64, ... of the segment, the 64 partial
//     sums meet in a six-step tree through LDS and lane 0 writes the XYZZ sum.  No wave waits for another workgroup, so a
//     segment of any length is summed correctly (a long one slowly: that is pg_msm's job).  An empty segment gives the identity.
//   * g1_normalize_kernel (msm.hpp) turns the n_segs x n_cols sums into affine points.
#pragma once

#include "fr.hpp"  // Fr, fr_from_mont
#include "g1.hpp"

#ifndef PG_MSM_SMALL_WINDOW
// W = 3: three table slots, 36 KiB of LDS per wave, four waves per CU (one per SIMD); W = 4 has 8 % fewer products and seven
// slots, 84 KiB: one wave per CU, and is 3.1 - 3.3 x slower at 2^10 and 2^14 segments of 27 points.
#define PG_MSM_SMALL_WINDOW 3
#endif

namespace pg {

constexpr uint32_t kSmallWindow = PG_MSM_SMALL_WINDOW;
constexpr uint32_t kSmallWindows = 255 / kSmallWindow + 1;         // 86 (W = 3), 64 (W = 4)
constexpr uint32_t kSmallTopBits = 256 - kSmallWindow * (kSmallWindows - 1);  // bits of the 256-bit span in the top window
constexpr uint32_t kSmallSlots = (1u << (kSmallWindow - 1)) - 1;   // 2 P .. 2^(W-1) P
constexpr uint32_t kSmallLanes = 64;                               // one wave per workgroup, in both kernels
static_assert(kSmallWindow >= 2 && kSmallWindow <= 4, "the table has to fit the LDS of one workgroup");
static_assert(255 - kSmallWindow * (kSmallWindows - 1) < kSmallWindow, "the top window must absorb its carry");
static_assert(kSmallWindows <= 128, "the carries are kept in two 64-bit masks");

// a point in LDS: word k of lane l's slot s at [(s 24 + k) 64 + l]
__device__ inline void lds_put_fq(uint64_t *at, const Fq &a) {
#pragma unroll
    for (int k = 0; k < 6; k++) at[k * kSmallLanes] = a.l[k];
}
__device__ inline Fq lds_get_fq(const uint64_t *at) {
    Fq a;
#pragma unroll
    for (int k = 0; k < 6; k++) a.l[k] = at[k * kSmallLanes];
    return a;
}
__device__ inline void lds_put_g1x(uint64_t *tab, uint32_t slot, uint32_t lane, const G1X &p) {
    uint64_t *at = tab + slot * 24 * kSmallLanes + lane;
    lds_put_fq(at, p.x);
    lds_put_fq(at + 6 * kSmallLanes, p.y);
    lds_put_fq(at + 12 * kSmallLanes, p.zz);
    lds_put_fq(at + 18 * kSmallLanes, p.zzz);
}
__device__ inline G1X lds_get_g1x(const uint64_t *tab, uint32_t slot, uint32_t lane) {
    const uint64_t *at = tab + slot * 24 * kSmallLanes + lane;
    return G1X{lds_get_fq(at), lds_get_fq(at + 6 * kSmallLanes), lds_get_fq(at + 12 * kSmallLanes), lds_get_fq(at + 18 * kSmallLanes)};
}

// prod[j n + i] = s_j[i] bases[i] (XYZZ) for i < n, j < n_cols; s_j = s + j col_stride
__global__ __launch_bounds__(kSmallLanes) void msm_seg_mul_kernel(const G1A *bases, const Fr *s, uint64_t n, uint64_t n_cols,
                                                                  uint64_t col_stride, G1X *prod) {
    constexpr uint32_t W = kSmallWindow, NW = kSmallWindows, HALF = 1u << (W - 1), MASK = (1u << W) - 1;
    __shared__ uint64_t tab[kSmallSlots * 24 * kSmallLanes];
    const uint32_t lane = threadIdx.x;
    const uint64_t t = (uint64_t)blockIdx.x * kSmallLanes + lane;
    if (t >= n * n_cols) return;  // (no barrier below: a lane reads only the slots it wrote)
    const uint64_t j = t / n, i = t - j * n;
    {
        const G1A p = bases[i];
        G1X m = g1x_from_affine(p);
#pragma unroll 1
        for (uint32_t k = 0; k < kSmallSlots; k++) {
            m = g1x_add_affine(m, p);  // (2 P: the complete addition doubles)
            lds_put_g1x(tab, k, lane, m);
        }
    }
    const Fr c = fr_from_mont(s[j * col_stride + i]);
    // carry INTO window k, from the bottom up: bit k of (clo, chi)
    uint64_t clo = 0, chi = 0;
    {
        uint64_t l0 = c.l[0], l1 = c.l[1], l2 = c.l[2], l3 = c.l[3];
        uint32_t carry = 0;
#pragma unroll 1
        for (uint32_t k = 0; k < NW; k++) {
            if (k < 64) clo |= (uint64_t)carry << k;
            else chi |= (uint64_t)carry << (k - 64);
            carry = ((uint32_t)l0 & MASK) + carry > HALF ? 1u : 0u;
            l0 = (l0 >> W) | (l1 << (64 - W));
            l1 = (l1 >> W) | (l2 << (64 - W));
            l2 = (l2 >> W) | (l3 << (64 - W));
            l3 >>= W;
        }
    }
    uint64_t l0 = c.l[0], l1 = c.l[1], l2 = c.l[2], l3 = c.l[3];
    G1X acc = g1x_identity();
#pragma unroll 1
    for (int k = (int)NW - 1; k >= 0; k--) {
        const uint32_t sh = k == (int)NW - 1 ? kSmallTopBits : W;  // the top window holds what is left of 256 bits
        if (k != (int)NW - 1) {
#pragma unroll 1
            for (uint32_t b = 0; b < W; b++) acc = g1x_dbl(acc);
        }
        const uint32_t cin = (uint32_t)((k < 64 ? clo >> k : chi >> (k - 64)) & 1);
        const uint32_t raw = (uint32_t)(l3 >> (64 - sh)) + cin;
        l3 = (l3 << sh) | (l2 >> (64 - sh));
        l2 = (l2 << sh) | (l1 >> (64 - sh));
        l1 = (l1 << sh) | (l0 >> (64 - sh));
        l0 <<= sh;
        const bool minus = raw > HALF;
        const uint32_t mag = minus ? (1u << W) - raw : raw;
        if (mag == 0) continue;
        G1X e;
        if (mag == 1) e = g1x_from_affine(bases[i]);
        else e = lds_get_g1x(tab, mag - 2, lane);
        if (minus) e.y = fq_neg(e.y);
        acc = g1x_add(acc, e);
    }
    prod[t] = acc;
}

// sums[seg n_cols + j] = the sum of prod[j n + i] over seg_off[seg] <= i < seg_off[seg + 1] (XYZZ); a workgroup (one wave)
// walks the pairs (seg, j) = blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(kSmallLanes) void msm_seg_sum_kernel(const G1X *prod, const uint64_t *seg_off, uint64_t n, uint64_t n_segs,
                                                                  uint64_t n_cols, G1X *sums) {
    __shared__ uint64_t tree[24 * kSmallLanes];
    const uint32_t lane = threadIdx.x;
#pragma unroll 1
    for (uint64_t pair = blockIdx.x; pair < n_segs * n_cols; pair += gridDim.x) {
        const uint64_t seg = pair / n_cols, j = pair - seg * n_cols;
        const uint64_t lo = seg_off[seg], hi = seg_off[seg + 1];
        const G1X *p = prod + j * n;
        G1X acc = g1x_identity();
#pragma unroll 1
        for (uint64_t i = lo + lane; i < hi; i += kSmallLanes) acc = g1x_add(acc, p[i]);
        // lanes beyond the segment hold the identity: a short segment's tree steps return at once for them
#pragma unroll 1
        for (uint32_t half = kSmallLanes / 2; half >= 1; half >>= 1) {
            if (lane >= half && lane < 2 * half) lds_put_g1x(tree, 0, lane, acc);
            __syncthreads();
            if (lane < half && lo + lane + half < hi) acc = g1x_add(acc, lds_get_g1x(tree, 0, lane + half));
            __syncthreads();
        }
        if (lane == 0) sums[pair] = acc;
    }
}

}  // namespace pg
