// permutation_product.hpp -- the copy permutation as field elements (gfx950): sigma evaluations and PLONK's grand product z.
//
// Over the domain H = <omega> of padded_n = 2^m rows, with coset constants k_0..k_3 (one per wire; the defaults [DEP-RECALL]
// are dusk-plonk 0.8's 1, K1 = 7, K2 = 13, K3 = 17) and sigma as pg_composer_permutation writes it (s = wire * padded_n + gate):
//   sigma evaluation of position p:   k[s >> m] * omega^(s & (padded_n - 1)),   s = sigma[p]
//   ratio of row i:                   num_i / den_i,   num_i = prod_j (w_j[i] + beta k_j omega^i + gamma),
//                                                      den_i = prod_j (w_j[i] + beta sigma_eval_j[i] + gamma)
//   z[i] = prod_{r < i} ratio_r (z[0] = 1),  wrap = prod_{r < padded_n} ratio_r  (== 1 iff the copy constraints hold, w.h.p.)
// The wire values of rows i >= n_values read as zero (dusk-plonk pads the witness vectors with zeros to the domain size).
//
// omega^g through two tables built per call (pp_tables_kernel): lo[t] = omega^t for the low L = min(m, 10) bits, held in LDS by
// every workgroup that reads it (32 KiB), and hi[j][h] = c_j omega^(h 2^L) for the high bits, in global memory (padded_n / 8 bytes:
// 64 MiB at 2^29, L2 / Infinity-Cache resident), with c_j = beta k_j for the product and c_j = k_j for the evaluations.  Then every
// c_j omega^g is ONE multiplication, hi[j][g >> L] * lo[g & (2^L - 1)].  Every index is masked: a sigma entry >= 4 padded_n raises
// the call's error flag and is looked up at s & (4 padded_n - 1), so a malformed sigma cannot read outside the tables.
//
// The product is three launches with no communication between workgroups inside one:
//   1. pp_ratio_kernel: a tile of kPpTile rows per workgroup step, lane t taking rows t, t + 256, ... (coalesced): num and den,
//      the ratios by Montgomery's trick over the lane's kPpRowsPerLane rows (one inversion per 64 rows), written over d_z; the
//      tile's product into tile_prod.  The running products of the trick go to memory, not registers: num_k * P_{k-1} into
//      d_z[row] and den_k into a per-workgroup scratch slab, read back by the same lane in the unwind.
//   2. pp_carry_kernel: one workgroup, the exclusive scan of the tile products (carry of each tile) and the total (*d_wrap).
//   3. pp_scan_kernel: a tile per workgroup, lane t owning kPpRowsPerLane CONSECUTIVE rows: product of its ratios, a scan of the
//      lanes' products in LDS, then z[i] = carry * prod of the earlier ratios, in place.
// A zero denominator raises the flag that makes the call return PG_ERR_NON_EXISTING_INVERSE (it is replaced by 1 so that the
// trick stays defined; the output is not meaningful then).
#pragma once

#include "emit.hpp"

namespace pg {

constexpr uint32_t kPpLoBitsMax = 10;                      // lo table: at most 1024 entries (32 KiB of LDS)
constexpr uint32_t kPpRowsPerLane = 64;                    // rows per lane per tile: one inversion per 64 rows
constexpr uint64_t kPpTile = (uint64_t)kThreads * kPpRowsPerLane;  // 16384 rows
constexpr uint32_t kPpFlagZeroDen = 1, kPpFlagBadSigma = 2;

// the tables' inputs: pw[b] = omega^(2^b), c[j] the wire's multiplier (kernel argument: 1152 bytes)
struct PpPowers {
    Fr pw[32];
    Fr c[4];
};

// lo[e] = omega^e for e < 2^L; hi[j * H + h] = c[j] * omega^(h 2^L) for h < H = padded_n >> L and j < nc (<= 4).  (pw[b] may be
// the powers of any base: ntt.hpp builds its tables of omega^x and of the coset generator's g^x here too.)
__global__ __launch_bounds__(kThreads) void pp_tables_kernel(const PpPowers P, uint32_t L, uint64_t H, uint32_t nc, uint4 *lo, uint4 *hi) {
    const uint64_t nlo = 1ull << L;
    for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < nlo + H; e += (uint64_t)gridDim.x * kThreads) {
        const bool low = e < nlo;
        const uint64_t x = low ? e : e - nlo;
        const uint32_t shift = low ? 0 : L;
        Fr acc = fr_one();
        for (uint32_t b = 0; b + shift < 32 && (x >> b); b++)
            if ((x >> b) & 1) acc = fr_mul(acc, P.pw[b + shift]);
        FrVec o;
        if (low) {
            o.f = acc;
            lo[2 * e] = o.v[0];
            lo[2 * e + 1] = o.v[1];
            continue;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (j >= nc) break;
            o.f = fr_mul(P.c[j], acc);
            hi[2 * (j * H + x)] = o.v[0];
            hi[2 * (j * H + x) + 1] = o.v[1];
        }
    }
}

__device__ __forceinline__ Fr pp_load(const uint4 *p, uint64_t i) {
    FrVec v;
    v.v[0] = p[2 * i];
    v.v[1] = p[2 * i + 1];
    return v.f;
}
__device__ __forceinline__ void pp_store(uint4 *p, uint64_t i, const Fr &f) {
    FrVec v;
    v.f = f;
    p[2 * i] = v.v[0];
    p[2 * i + 1] = v.v[1];
}

// the domain and its tables as one kernel argument
struct PpDomain {
    uint64_t padded_n, H;  // H = padded_n >> L
    uint32_t m, L;
    const uint4 *lo, *hi;
};

// every workgroup's copy of the lo table
__device__ __forceinline__ void pp_lo_to_lds(const PpDomain &D, FrVec *lo_s) {
    for (uint32_t e = threadIdx.x; e < (1u << D.L); e += kThreads) lo_s[e].f = pp_load(D.lo, e);
    __syncthreads();
}

// c_j omega^g, j < 4 and g < padded_n (the caller masks both)
__device__ __forceinline__ Fr pp_pow(const PpDomain &D, const FrVec *lo_s, uint32_t j, uint64_t g) {
    return fr_mul(pp_load(D.hi, j * D.H + (g >> D.L)), lo_s[g & ((1u << D.L) - 1)].f);
}

// sigma entry -> (wire, gate), masked into the domain; a bad entry raises the flag
__device__ __forceinline__ void pp_split(const PpDomain &D, uint64_t s, uint32_t &j, uint64_t &g, uint32_t *flags) {
    if (s >> (D.m + 2)) {
        atomicOr(flags, kPpFlagBadSigma);
        s &= (4ull << D.m) - 1;
    }
    j = (uint32_t)(s >> D.m);
    g = s & (D.padded_n - 1);
}

// out[p] = k[s >> m] omega^(s mod padded_n), s = sigma[p], p < 4 padded_n
__global__ __launch_bounds__(kThreads) void pp_sigma_eval_kernel(const PpDomain D, const uint64_t *sigma, uint4 *out, uint32_t *flags) {
    __shared__ FrVec lo_s[1u << kPpLoBitsMax];
    pp_lo_to_lds(D, lo_s);
    const uint64_t total = 4 * D.padded_n;
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < total; p += (uint64_t)gridDim.x * kThreads) {
        uint32_t j;
        uint64_t g;
        pp_split(D, sigma[p], j, g, flags);
        pp_store(out, p, pp_pow(D, lo_s, j, g));
    }
}

// 256 lanes' values -> lane t gets the product of lanes < t (exclusive; 1 for lane 0) and the product of all 256.
// buf: 2 x 256 entries of LDS.  Every lane of the workgroup calls it.
struct PpScan {
    Fr before, total;
};
__device__ __forceinline__ PpScan pp_block_exclusive_scan(const Fr &x, FrVec *buf) {
    const uint32_t t = threadIdx.x;
    uint32_t cur = 0;
    Fr v = x;
    buf[t].f = v;
    __syncthreads();
#pragma unroll
    for (uint32_t off = 1; off < kThreads; off <<= 1) {
        if (t >= off) v = fr_mul(buf[cur + t - off].f, v);
        cur ^= kThreads;
        buf[cur + t].f = v;
        __syncthreads();
    }
    PpScan r;
    r.before = t ? buf[cur + t - 1].f : fr_one();
    r.total = buf[cur + kThreads - 1].f;
    __syncthreads();  // (buf is reused by the caller's next scan)
    return r;
}

struct PpProduct {
    PpDomain D;
    const uint4 *w[4];       // wire values, n_values entries each
    uint64_t n_values;
    const uint64_t *sigma;   // 4 x padded_n
    Fr gamma;
    uint4 *z;                // padded_n: ratios after launch 1, z after launch 3
    uint4 *den;              // gridDim.x (launch 1) x kPpTile: the unwind's denominators
    uint4 *tile_prod;        // tiles
    uint4 *tile_carry;       // tiles
    uint4 *wrap;             // 1
    uint64_t tiles;
    uint32_t *flags;
};

// launch 1 (see the top of the file)
__global__ __launch_bounds__(kThreads) void pp_ratio_kernel(const PpProduct A) {
    __shared__ FrVec lo_s[1u << kPpLoBitsMax];
    __shared__ FrVec scan[2 * kThreads];
    const PpDomain &D = A.D;
    pp_lo_to_lds(D, lo_s);
    const uint32_t t = threadIdx.x;
    uint4 *den_slab = A.den + 2 * (uint64_t)blockIdx.x * kPpTile;
#pragma unroll 1
    for (uint64_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const uint64_t base = tile * kPpTile;
        Fr P = fr_one(), N = fr_one();  // running product of the denominators / of the numerators
#pragma unroll 1
        for (uint32_t k = 0; k < kPpRowsPerLane; k++) {
            const uint64_t row = base + (uint64_t)k * kThreads + t;
            if (row >= D.padded_n) break;
            Fr num = fr_one(), den = fr_one();
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const Fr wg = fr_add(row < A.n_values ? pp_load(A.w[j], row) : fr_zero(), A.gamma);
                uint32_t sj;
                uint64_t sg;
                pp_split(D, A.sigma[j * D.padded_n + row], sj, sg, A.flags);
                const Fr n = fr_add(wg, pp_pow(D, lo_s, j, row));
                const Fr d = fr_add(wg, pp_pow(D, lo_s, sj, sg));
                num = j ? fr_mul(num, n) : n;
                den = j ? fr_mul(den, d) : d;
            }
            if (fr_is_zero(den)) {
                atomicOr(A.flags, kPpFlagZeroDen);
                den = fr_one();
            }
            pp_store(A.z, row, fr_mul(num, P));  // num_k * P_{k-1}
            pp_store(den_slab, (uint64_t)k * kThreads + t, den);
            P = fr_mul(P, den);
            N = fr_mul(N, num);
        }
        Fr I = fr_invert_or_zero(P);           // 1 / P_{last}
        const Fr lane_prod = fr_mul(N, I);     // the product of this lane's ratios
        for (int k = (int)kPpRowsPerLane - 1; k >= 0; k--) {
            const uint64_t row = base + (uint64_t)k * kThreads + t;
            if (row >= D.padded_n) continue;
            const Fr x = pp_load(A.z, row);
            const Fr den = pp_load(den_slab, (uint64_t)k * kThreads + t);
            pp_store(A.z, row, fr_mul(x, I));  // num_k * P_{k-1} / P_k
            I = fr_mul(I, den);                // 1 / P_{k-1}
        }
        const PpScan sc = pp_block_exclusive_scan(lane_prod, scan);
        if (t == 0) pp_store(A.tile_prod, tile, sc.total);
    }
}

// launch 2: one workgroup
__global__ __launch_bounds__(kThreads) void pp_carry_kernel(const PpProduct A) {
    __shared__ FrVec scan[2 * kThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (A.tiles + kThreads - 1) / kThreads, lo = t * per, hi = lo + per < A.tiles ? lo + per : A.tiles;
    Fr p = fr_one();
    for (uint64_t i = lo; i < hi; i++) p = fr_mul(p, pp_load(A.tile_prod, i));
    const PpScan sc = pp_block_exclusive_scan(p, scan);
    Fr acc = sc.before;
    for (uint64_t i = lo; i < hi; i++) {
        const Fr x = pp_load(A.tile_prod, i);
        pp_store(A.tile_carry, i, acc);
        acc = fr_mul(acc, x);
    }
    if (t == 0) pp_store(A.wrap, 0, sc.total);
}

// launch 3: one tile per workgroup
__global__ __launch_bounds__(kThreads) void pp_scan_kernel(const PpProduct A) {
    __shared__ FrVec scan[2 * kThreads];
    const uint64_t first = blockIdx.x * kPpTile + (uint64_t)threadIdx.x * kPpRowsPerLane;
    const uint64_t end = first + kPpRowsPerLane < A.D.padded_n ? first + kPpRowsPerLane : A.D.padded_n;
    Fr p = fr_one();
    for (uint64_t i = first; i < end; i++) p = fr_mul(p, pp_load(A.z, i));
    Fr acc = fr_mul(pp_load(A.tile_carry, blockIdx.x), pp_block_exclusive_scan(p, scan).before);
    for (uint64_t i = first; i < end; i++) {
        const Fr r = pp_load(A.z, i);
        pp_store(A.z, i, acc);
        acc = fr_mul(acc, r);
    }
}

}  // namespace pg
