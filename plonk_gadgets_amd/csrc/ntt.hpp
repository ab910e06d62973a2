// ntt.hpp -- number-theoretic transforms over the scalar field (gfx950): dusk-plonk 0.8's EvaluationDomain::{fft, ifft, coset_fft,
// coset_ifft} on n = 2^m points, m <= 32, for n_cols columns at a fixed stride, in place, natural order in and out.
//   fft:        e_j = sum_i c_i omega^(ij)               ifft:       c_i = n^-1 sum_j e_j omega^(-ij)
//   coset_fft:  fft(c_i g^i)                             coset_ifft: g^-i ifft(e)_i
//
// The transform is radix-2 decimation in frequency (natural order in, bit-reversed out), grouped into passes of at most 2^10
// points, then one bit-reversal pass:
//   * A pass on blocks of N = 2^bp contiguous points does, for each column c < S = N / R of a block (the points c + S t, t < R = 2^k),
//     the R-point DFT over t in LDS (k radix-2 stages, roots omega_R^e = omega^(e n / R) in LDS), then multiplies output u by the
//     twiddle omega_N^(c u) = omega^((n / N) c u), and writes it back where it was read.  The block's output u is then the first
//     digit of the remaining transform of the contiguous block at S rev_k(u) (four-step recursion): after the passes, position p
//     holds e_{rev_m(p)}.  The first pass has N = n, the last N = R = 2^10 (no twiddle); the strided ones between take R <= 2^7 and
//     2^(10 - k) >= 8 ADJACENT columns per tile, so that every row of a tile is at least 256 contiguous bytes.  m <= 10: one pass,
//     which writes its output straight to the natural positions.
//   * ntt_reverse_kernel swaps the 32 x 32 tiles (a, mid, c) <-> (rev(c), rev(mid), rev(a)) of the index's top 5, middle m - 10
//     and low 5 bits through LDS: rows of 32 contiguous points (1 KiB) on both sides, no scattered 32-byte accesses.
//   * omega^x (x < n) is ONE multiplication through two tables built per call by pp_tables_kernel (permutation_product.hpp):
//     lo[x mod 2^L] * hi[x >> L], L = min(m, 10).  The coset's g^i (and n^-1 g^-i) comes from two more such tables; the coset
//     scaling is folded into the first pass's loads, the n^-1 and g^-i scalings into the stores of the bit-reversal pass (or of
//     the single pass).  The inverse kinds run the same passes with omega^-1.
// Device memory a call keeps (the engine's, grow-only): the tables, (2^L + n / 2^L) x 32 bytes each, one for fft / ifft and two
// for the coset kinds: 64 MiB + 64 MiB at n = 2^31.  LDS: 48 KiB per pass workgroup (a 1024-point tile and 512 roots), 66 KiB per
// bit-reversal workgroup.  No index is narrower than 64 bits where it can reach n_cols x stride or n.
#pragma once

#include "permutation_product.hpp"

namespace pg {

constexpr uint32_t kNttTileBits = 10;   // points per pass tile: 1024 (32 KiB of LDS)
constexpr uint32_t kNttStridedBits = 7;  // a strided pass: R <= 2^7 points per column, >= 8 adjacent columns per tile
constexpr uint32_t kNttRevBits = 5;      // the bit-reversal tiles: 32 x 32 points
constexpr uint32_t kNttRevPad = 33;      // (LDS row pitch of those tiles, in points)

// base^x for x < 2^m through the two tables of pp_tables_kernel (the host built them for the same L and m)
struct NttTable {
    const uint4 *lo, *hi;  // lo == nullptr: no table
    uint32_t L;
};
__device__ __forceinline__ Fr ntt_pow(const NttTable &T, uint64_t x) {
    return fr_mul(pp_load(T.hi, x >> T.L), pp_load(T.lo, x & ((1ull << T.L) - 1)));
}

__device__ __forceinline__ uint32_t ntt_rev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32 - bits) : 0; }

struct NttPass {
    uint4 *data;              // column j at data + 2 * j * stride (points of 32 bytes)
    const uint4 *src;         // non-NULL: the first pass reads its column j at src + 2 * j * stride instead (out of place)
    uint64_t n_cols, stride;
    uint32_t m, bp, k, cb;    // log2 of: n, the block, R (points per column of a tile), the adjacent columns per tile
    uint32_t twiddle;         // multiply output u of column c by omega^((n / N) c u): every pass but the last
    uint32_t natural;         // m <= 10: the only pass, which stores output u at position u and applies `post`
    NttTable w;               // omega^x (omega^-1 for the inverse kinds)
    NttTable pre;             // first pass of coset_fft: g^i on the loads
    NttTable post;            // coset_ifft: n^-1 g^-i on the final stores
    Fr scale;                 // ifft: n^-1 on the final stores (use_scale)
    uint32_t use_scale;
};

// the final store's factor for natural index i
__device__ __forceinline__ Fr ntt_post(const NttPass &P, uint64_t i, const Fr &x) {
    if (P.post.lo) return fr_mul(x, ntt_pow(P.post, i));
    if (P.use_scale) return fr_mul(x, P.scale);
    return x;
}

// one pass: a tile (R rows x C = 2^cb adjacent columns of one block) per workgroup step; tile point e = t * C + cc
__global__ __launch_bounds__(kThreads) void ntt_pass_kernel(const NttPass P) {
    __shared__ FrVec tile[1u << kNttTileBits];
    __shared__ FrVec root[1u << (kNttTileBits - 1)];
    const uint32_t k = P.k, cb = P.cb, C = 1u << cb, T = 1u << (k + cb);
    const uint64_t n_mask = (1ull << P.m) - 1;
    for (uint32_t e = threadIdx.x; e < (1u << k) / 2; e += kThreads) root[e].f = ntt_pow(P.w, ((uint64_t)e << (P.m - k)) & n_mask);
    const uint64_t S = 1ull << (P.bp - k);               // columns of a block
    const uint32_t gbits = P.bp - k - cb, tbits = P.m - k - cb;  // log2 of: column groups per block, tiles per column
    const uint64_t tiles = P.n_cols << tbits;
#pragma unroll 1
    for (uint64_t tau = blockIdx.x; tau < tiles; tau += gridDim.x) {
        const uint64_t col = tau >> tbits, r = tau & ((1ull << tbits) - 1);
        const uint64_t first = ((r >> gbits) << P.bp) + ((r & ((1ull << gbits) - 1)) << cb);  // index of point (0, 0) in the column
        const uint64_t c0 = first & (S - 1);
        uint4 *base = P.data + 2 * (col * P.stride + first);
        const uint4 *in = P.src ? P.src + 2 * (col * P.stride + first) : base;
        for (uint32_t e = threadIdx.x; e < T; e += kThreads) {
            const uint64_t off = (e & (C - 1)) + S * (e >> cb);
            Fr x = pp_load(in, off);
            if (P.pre.lo) x = fr_mul(x, ntt_pow(P.pre, first + off));
            tile[e].f = x;
        }
        __syncthreads();
#pragma unroll 1
        for (uint32_t s = 0; s < k; s++) {
            const uint32_t h = (1u << k) >> (s + 1);
            for (uint32_t b = threadIdx.x; b < T / 2; b += kThreads) {
                const uint32_t cc = b & (C - 1), jj = b >> cb, j = jj & (h - 1);
                const uint32_t ia = ((((jj - j) << 1) + j) << cb) + cc, ib = ia + (h << cb);
                const Fr x = tile[ia].f, y = tile[ib].f;
                tile[ia].f = fr_add(x, y);
                const Fr d = fr_sub(x, y);
                tile[ib].f = h > 1 ? fr_mul(d, root[j << s].f) : d;  // (the last stage's roots are all one)
            }
            __syncthreads();
        }
        for (uint32_t e = threadIdx.x; e < T; e += kThreads) {
            const uint32_t cc = e & (C - 1), t = e >> cb, u = ntt_rev(t, k);
            Fr x = tile[e].f;
            if (P.natural) {  // bp = k = m, cb = 0: the whole transform; output u goes to position u
                pp_store(base, u, ntt_post(P, u, x));
                continue;
            }
            if (P.twiddle) x = fr_mul(x, ntt_pow(P.w, (((c0 + cc) * u) << (P.m - P.bp)) & n_mask));
            pp_store(base, cc + S * t, x);
        }
        __syncthreads();  // (the tile is reused)
    }
}

// position p holds e_{rev_m(p)} -> natural order, with the final scaling; m > 2 * kNttRevBits.  One pair of tiles (mid, rev(mid)) per
// workgroup step; the step of the larger of the two does nothing.
__global__ __launch_bounds__(kThreads) void ntt_reverse_kernel(const NttPass P) {
    constexpr uint32_t W = 1u << kNttRevBits;
    __shared__ FrVec sa[W * kNttRevPad], sb[W * kNttRevPad];
    const uint32_t mb = P.m - 2 * kNttRevBits, hs = P.m - kNttRevBits;
    const uint64_t tiles = P.n_cols << mb;
#pragma unroll 1
    for (uint64_t tau = blockIdx.x; tau < tiles; tau += gridDim.x) {
        const uint64_t col = tau >> mb;
        const uint32_t mid = (uint32_t)(tau & ((1ull << mb) - 1)), mr = ntt_rev(mid, mb);
        if (mr < mid) continue;  // (uniform over the workgroup)
        uint4 *base = P.data + 2 * col * P.stride;
        const uint64_t ma = (uint64_t)mid << kNttRevBits, mra = (uint64_t)mr << kNttRevBits;
        for (uint32_t e = threadIdx.x; e < W * W; e += kThreads) {
            const uint32_t a = e >> kNttRevBits, c = e & (W - 1);
            sa[a * kNttRevPad + c].f = pp_load(base, ((uint64_t)a << hs) + ma + c);
            if (mr != mid) sb[a * kNttRevPad + c].f = pp_load(base, ((uint64_t)a << hs) + mra + c);
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < W * W; e += kThreads) {
            const uint32_t a = e >> kNttRevBits, c = e & (W - 1);
            const uint32_t src = ntt_rev(c, kNttRevBits) * kNttRevPad + ntt_rev(a, kNttRevBits);
            const uint64_t d = ((uint64_t)a << hs) + mra + c;  // point (a, c) of tile rev(mid) <- (rev(c), rev(a)) of tile mid
            pp_store(base, d, ntt_post(P, d, sa[src].f));
            if (mr != mid) {
                const uint64_t d2 = ((uint64_t)a << hs) + ma + c;
                pp_store(base, d2, ntt_post(P, d2, sb[src].f));
            }
        }
        __syncthreads();
    }
}

}  // namespace pg
