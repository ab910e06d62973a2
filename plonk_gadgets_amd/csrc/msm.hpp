// msm.hpp -- commitments over BLS12-381 G1 (gfx950): the Pippenger multi-scalar multiplication of pg_msm, the insecure
// development SRS of pg_srs_setup, and batch normalisation to affine points.
//
// MSM, per scalar column (capi_msm.inc enqueues):
//   * signed 16-bit digits: 16 windows of c = 16 bits.  Window w's raw value r (bits 16w..16w+15 plus the carry of window
//     w - 1) becomes r when r <= 2^15, else r - 2^16 with a carry into window w + 1.  A scalar < r_Fr < 2^255 leaves window
//     15 at most 2^15 - 1 + 1, so the carry out of the last window is always 0: 16 windows cover every scalar.  The bucket
//     of a digit is |d| in [0, 2^15]; 0 is no bucket.  msm_digits_kernel writes, per window, |d| << 32 | sign << 31 | i.
//   * rocprim::radix_sort_keys over bits 32..47 groups the window's points by bucket (no atomics on points).
//   * segmented bucket sums, msm_segsum_kernel: lane t sums kMsmRun consecutive sorted entries run by run.  A run that starts
//     and ends inside the lane's chunk is a whole bucket: bucket[key] += sum.  A run that is cut by the chunk's first or last
//     entry leaves a partial in one of the lane's two output slots (key, point); a slot with nothing to say holds the
//     identity under a real key, so the slots are sorted by key again and the same kernel runs on them, 2 / kMsmRun as many
//     entries, until one chunk holds everything.  No lane adds more than kMsmRun points per launch, whatever the digits
//     (a single hot bucket included).  A bucket is written by at most one lane per launch and launches are ordered.
//   * msm_bucket_reduce_kernel: sum_k k B_k per window through running sums over kMsmSegs segments of kMsmSegLen buckets,
//     each finished with (a - 1) T for its first index a and total T; msm_window_kernel adds a window's segments;
//     msm_combine_kernel runs Horner over the windows (16 doublings per window).
//   * g1_normalize_kernel: one inversion per lane's batch (Montgomery's trick), identity -> (0, 0).
//
// SRS: tau^i base for i < n.  A fixed-base table T[w][d] = d 2^(8w) base (32 windows of 8 bits, d < 256) is built and
// normalised once; lane i then computes tau^i (a power from the table of tau^(2^b), then one product per further point of its
// run) and sums the 32 table entries its canonical bytes select.  Chunks of kSrsChunk points go through an XYZZ workspace and
// g1_normalize_kernel.
#pragma once

#include <rocprim/rocprim.hpp>

#include "emit.hpp"  // kThreads
#include "g1.hpp"

namespace pg {

constexpr uint32_t kMsmWindows = 16;               // c = 16: 16 windows of a 256-bit span
constexpr uint32_t kMsmBuckets = 1u << 15;         // bucket indices 1 .. 2^15 (index 0: digit 0, skipped)
constexpr uint32_t kMsmRun = 64;                   // sorted entries per lane in msm_segsum_kernel
constexpr uint32_t kMsmSegs = 256;                 // bucket segments per window in the reduction
constexpr uint32_t kMsmSegLen = kMsmBuckets / kMsmSegs;
constexpr uint32_t kMsmSmallThreads = 64;          // the reduction's and the tail's workgroups
constexpr uint64_t kSrsChunk = 1ull << 21;         // points per SRS chunk (XYZZ workspace: 384 MiB)
constexpr uint32_t kSrsPerLane = 16;               // SRS points per lane (one power from the table, then products)
constexpr uint32_t kNormPerLane = 32;              // points per inversion in g1_normalize_kernel

struct FrPow2 {
    Fr pw[32];  // tau^(2^b)
};

// pairs[i] = |d_w(s_i)| << 32 | (d_w(s_i) < 0) << 31 | i for window w (Montgomery-form scalars, converted here).  One 64-bit
// key per point, sorted on its bits 32..47 (radix_sort_keys: the instantiation permutation.hpp's sort already uses; rocPRIM's
// pairs sort of 32-bit keys and values keeps 80 bytes of scratch per lane on gfx950)
__global__ __launch_bounds__(kThreads) void msm_digits_kernel(const Fr *s, uint64_t n, uint32_t w, uint64_t *pairs) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const Fr c = fr_from_mont(s[i]);
        uint64_t l0 = c.l[0], l1 = c.l[1], l2 = c.l[2], l3 = c.l[3];
        uint32_t carry = 0, raw = 0;
#pragma unroll 1
        for (uint32_t j = 0; j <= w; j++) {
            raw = ((uint32_t)l0 & 0xffffu) + carry;
            carry = raw > (1u << 15) ? 1u : 0u;
            l0 = (l0 >> 16) | (l1 << 48);
            l1 = (l1 >> 16) | (l2 << 48);
            l2 = (l2 >> 16) | (l3 << 48);
            l3 >>= 16;
        }
        pairs[i] = (uint64_t)(carry ? (1u << 16) - raw : raw) << 32 | carry << 31 | (uint32_t)i;
    }
}

// one launch of the segmented sums; AFFINE: the first level (the sorted 64-bit pairs of msm_digits_kernel over `bases`), else
// a level of partials (keys, pts).  Lane t owns entries [t kMsmRun, min(m, (t + 1) kMsmRun)) and output slots 2t (the run cut
// at the chunk's start) and 2t + 1 (the run cut at its end).
template <bool AFFINE>
__global__ __launch_bounds__(kThreads) void msm_segsum_kernel(const uint64_t *pairs, const uint32_t *keys, const G1A *bases, const G1X *pts,
                                                              uint64_t m, G1X *buckets, uint32_t *okeys, G1X *opts) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x, s = t * kMsmRun;
    if (s >= m) return;
    const uint64_t e = s + kMsmRun < m ? s + kMsmRun : m;
    auto key = [&](uint64_t i) -> uint32_t {
        if constexpr (AFFINE) return (uint32_t)(pairs[i] >> 32);
        else return keys[i];
    };
    uint32_t cur = key(s);
    const bool head_open = s > 0 && key(s - 1) == cur;
    okeys[2 * t] = cur;
    okeys[2 * t + 1] = key(e - 1);
    opts[2 * t] = g1x_identity();
    opts[2 * t + 1] = g1x_identity();
    bool first = true;
    G1X acc = g1x_identity();
#pragma unroll 1
    for (uint64_t i = s; i <= e; i++) {
        const bool last = i == e;
        const uint32_t k = last ? 0 : key(i);
        if (last || k != cur) {
            const bool open_left = first && head_open, open_right = last && e < m && key(e) == cur;
            if (open_left) opts[2 * t] = acc;
            else if (open_right) opts[2 * t + 1] = acc;
            else if (cur != 0 && !g1x_is_identity(acc)) buckets[cur] = g1x_add(buckets[cur], acc);
            if (last) break;
            first = false;
            cur = k;
            acc = g1x_identity();
        }
        if constexpr (AFFINE) {
            if (k != 0) {
                const uint32_t v = (uint32_t)pairs[i];
                G1A p = bases[v & 0x7fffffffu];
                if (v >> 31) p = g1a_neg(p);
                acc = g1x_add_affine(acc, p);
            }
        } else {
            acc = g1x_add(acc, pts[i]);
        }
    }
}

// seg[w kMsmSegs + j] = sum over the segment's buckets k in [a, a + kMsmSegLen) of k B_k, a = 1 + j kMsmSegLen
__global__ __launch_bounds__(kMsmSmallThreads) void msm_bucket_reduce_kernel(const G1X *buckets, G1X *seg) {
    const uint32_t t = blockIdx.x * kMsmSmallThreads + threadIdx.x;
    if (t >= kMsmWindows * kMsmSegs) return;
    const uint32_t w = t / kMsmSegs, j = t % kMsmSegs, a = 1 + j * kMsmSegLen;
    const G1X *B = buckets + (uint64_t)w * (kMsmBuckets + 1);
    G1X sum = g1x_identity(), acc = g1x_identity();
#pragma unroll 1
    for (uint32_t k = a + kMsmSegLen - 1; k >= a; k--) {
        sum = g1x_add(sum, B[k]);
        acc = g1x_add(acc, sum);  // acc = sum_k (k - a + 1) B_k
    }
    seg[t] = g1x_add(acc, g1x_mul_small(sum, a - 1));
}

// win[w] = the sum of window w's segments
__global__ __launch_bounds__(kMsmSmallThreads) void msm_window_kernel(const G1X *seg, G1X *win) {
    const uint32_t w = threadIdx.x;
    if (w >= kMsmWindows) return;
    G1X acc = g1x_identity();
#pragma unroll 1
    for (uint32_t j = 0; j < kMsmSegs; j++) acc = g1x_add(acc, seg[w * kMsmSegs + j]);
    win[w] = acc;
}

// *out = sum_w 2^(16 w) win[w] (one lane)
__global__ __launch_bounds__(kMsmSmallThreads) void msm_combine_kernel(const G1X *win, G1X *out) {
    if (threadIdx.x != 0) return;
    G1X acc = win[kMsmWindows - 1];
#pragma unroll 1
    for (int w = (int)kMsmWindows - 2; w >= 0; w--) {
#pragma unroll 1
        for (int b = 0; b < 16; b++) acc = g1x_dbl(acc);
        acc = g1x_add(acc, win[w]);
    }
    *out = acc;
}

// out[i] = the affine form of in[i] for i < m; lane t normalises points [t per_lane, (t + 1) per_lane) with one inversion.
// The running products of Montgomery's trick are parked in out[i].x and read back by the same lane.
__global__ __launch_bounds__(kThreads) void g1_normalize_kernel(const G1X *in, G1A *out, uint64_t m, uint32_t per_lane) {
    const uint64_t s = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * per_lane;
    if (s >= m) return;
    const uint64_t e = s + per_lane < m ? s + per_lane : m;
    Fq acc = fq_one();
#pragma unroll 1
    for (uint64_t i = s; i < e; i++) {
        const Fq zz = in[i].zz;
        if (fq_is_zero(zz)) continue;
        out[i].x = acc;
        acc = fq_mul(acc, fq_mul(zz, in[i].zzz));
    }
    Fq inv = fq_invert(acc);
#pragma unroll 1
    for (uint64_t i = e; i-- > s;) {
        const G1X p = in[i];
        if (fq_is_zero(p.zz)) {
            out[i] = g1a_identity();
            continue;
        }
        const Fq d = fq_mul(p.zz, p.zzz), di = fq_mul(inv, out[i].x);  // 1 / (ZZ ZZZ)
        inv = fq_mul(inv, d);
        out[i] = G1A{fq_mul(p.x, fq_mul(di, p.zzz)), fq_mul(p.y, fq_mul(di, p.zz))};
    }
}

// table[w 256 + d] = d 2^(8w) base (XYZZ), w < 32, d < 256
__global__ __launch_bounds__(kThreads) void srs_table_kernel(const G1A base, G1X *table) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= 32 * 256) return;
    const uint32_t w = t >> 8, d = t & 255;
    G1X b = g1x_from_affine(base);
#pragma unroll 1
    for (uint32_t i = 0; i < 8 * w; i++) b = g1x_dbl(b);
    table[t] = g1x_mul_small(b, d);
}

// out[i - start] = tau^i base (XYZZ) for i in [start, start + count): lane t takes kSrsPerLane consecutive i
__global__ __launch_bounds__(kThreads) void srs_points_kernel(const G1A *table, const FrPow2 P, uint64_t start, uint64_t count, G1X *out) {
    const uint64_t s = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * kSrsPerLane;
    if (s >= count) return;
    const uint64_t e = s + kSrsPerLane < count ? s + kSrsPerLane : count, i0 = start + s;
    Fr pw = fr_one();
#pragma unroll 1
    for (uint32_t b = 0; b < 32; b++)
        if ((i0 >> b) & 1) pw = fr_mul(pw, P.pw[b]);
#pragma unroll 1
    for (uint64_t i = s; i < e; i++) {
        const Fr c = fr_from_mont(pw);
        uint64_t l0 = c.l[0], l1 = c.l[1], l2 = c.l[2], l3 = c.l[3];
        G1X acc = g1x_identity();
#pragma unroll 1
        for (uint32_t w = 0; w < 32; w++) {
            const uint32_t d = (uint32_t)l0 & 255u;
            if (d) acc = g1x_add_affine(acc, table[w * 256 + d]);
            l0 = (l0 >> 8) | (l1 << 56);
            l1 = (l1 >> 8) | (l2 << 56);
            l2 = (l2 >> 8) | (l3 << 56);
            l3 >>= 8;
        }
        out[i] = acc;
        pw = fr_mul(pw, P.pw[0]);
    }
}

}  // namespace pg
