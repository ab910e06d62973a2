// quotient.hpp -- the prover's round 3 and round 4 over the scalar field (gfx950): PLONK's quotient polynomial t(X) and the
// evaluation of polynomials at a point.
//
// The quotient, with the conventions [DEP-RECALL] of dusk-plonk 0.8's quotient_poly::compute: n = 2^m
// points of H = <omega>, zeta a primitive 4n-th root of unity with zeta^4 = omega, g the coset generator, k_0..k_3 the wires'
// coset constants; every input a polynomial of n coefficients.  At x on the coset g<zeta> (4n points)
//   N(x) = q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c) + PI
//        + alpha [ prod_j (w_j + beta k_j x + gamma) z(x) - prod_j (w_j + beta sigma_j + gamma) z(omega x) ]
//        + alpha^2 (z(x) - 1) L1(x),         L1(x) = (x^n - 1) / (n (x - 1))
// and t is the polynomial of degree < 4n with t(x) = N(x) / (x^n - 1) on those points, returned as t_lo | t_mid | t_hi | t_4th.
//
// The 4n points are four cosets of H: chunk j (j < 4) holds x = g_j omega^i, g_j = g zeta^j, i < n.  So every transform is an
// n-point one of ntt.hpp (a polynomial of degree < n needs no folding), z(omega x) is entry (i + 1) mod n of the same chunk, and
// x^n - 1 = c_j = g^n zeta^(jn) - 1 is a constant of the chunk.  Per chunk, the host (capi.hip, pg_quotient) enqueues:
//   * coset-forward transforms with g_j, out of place (the first pass reads the caller's coefficients), of a, b, c, d and z into
//     scratch columns 0..4, which stay for the whole chunk; the selectors and sigmas stream through columns 5..7;
//   * quotient_step_kernel<QS_*> launches that accumulate N / c_j into chunk j of d_t (the order below);
//   * after the four chunks, a coset-inverse transform of each chunk with g_j, in place: coefficient k0 of chunk j is then
//     r_j = sum_k1 t[k0 + n k1] g^(n k1) zeta^(j n k1), and quotient_combine_kernel inverts that 4-point DFT (root zeta^n) per k0
//     and multiplies by 4^-1 g^(-n k1), in place.
// x is ONE multiplication through pp_tables_kernel's two tables (lo[e] = omega^e, hi[h] = g_j omega^(h 2^L)).  The 1 / (n (x - 1))
// of L1 comes from Montgomery's trick per lane over kQRowsPerLane points (as pp_ratio_kernel does): the running products go to
// d_t and are read back by the same lane, and n (x - 1) is recomputed from the table instead of being stored.  x - 1 and c_j are
// never zero once the host has checked g^(4n) != 1, so nothing on the device can fail.
// No scratch memory, no LDS; 64-bit indices wherever one can reach 4n.
//
// The blinded quotient (pg_quotient_blinded): wire j has n + 2 coefficients, w_j = w_j0 + (b1 X + b0)(X^n - 1),
// and z has n + 3, z = z0 + (b2 X^2 + b1 X + b0)(X^n - 1), each a plain coefficient array whose rows n.. (the tail) hold the
// blinders.  On chunk j, x^n = c_j + 1 is a constant, so the values of a blinded column are the n-point coset transform of its
// rows 0..n-1 plus (c_j + 1) tail(x): step QS_BLIND (quotient_blind_kernel) adds that to scratch columns 0..4 after their
// transforms and before QS_PERM_NUM, and the six steps above run as they are.  N now has degree <= 5n + 6 and t = N / (X^n - 1)
// degree <= 4n + 6, so the 4n points give t~ = t mod (X^(4n) - g^(4n)): t~[k] = t[k] + g^(4n) t[4n + k] for k < 7.  With
// t (X^n - 1) = N, t[4n + i] = N[5n + i] = T_i (i < 7, n >= 7), and only the two permutation products reach degree 5n: their top
// seven coefficients are the truncated products of the top seven coefficients of their five factors (rows n+2..n-4 of z, times
// omega^row for z(omega X); rows n+1..n-5 of w_j, plus beta sigma_j from row n-1 down; beta k_j X + gamma lie below for n >= 8).
// quotient_top_kernel does that on one lane after the combine: t[4n + i] = T_i, t[4n + 7] = 0, t[k] -= g^(4n) T_k.
//
// The evaluation (pg_poly_evaluate): sum_{i < n} c_i x^i for n_cols columns at a stride, any n from 1 to 2^32.  A segment of
// kEvalSeg points per workgroup step: lane t reads points s + 256 k + t (coalesced) and runs Horner along them (acc = acc x^256
// + c: one multiplication per coefficient), multiplies by x^t (a 256-entry table) and the workgroup sums the lanes in LDS; lane 0
// multiplies by x^s (a table over the segments) and writes the segment's partial sum.  poly_eval_reduce_kernel sums a column's
// partials.
#pragma once

#include "ntt.hpp"

namespace pg {

constexpr uint32_t kQRowsPerLane = 32;                               // Montgomery's trick: one inversion per 32 points
constexpr uint64_t kQTile = (uint64_t)kThreads * kQRowsPerLane;      // 8192 points
constexpr uint32_t kEvalPerLane = 64;                                // Horner steps per lane and segment
constexpr uint64_t kEvalSeg = (uint64_t)kThreads * kEvalPerLane;     // 16384 points per segment

// the pointwise steps of one chunk, in launch order, and the scratch columns (s[0..7]) each reads
enum : int {
    QS_PERM_NUM = 0,  // t  = alpha z prod_j (w_j + beta k_j x + gamma) + alpha^2 c_j (z - 1) / (n (x - 1))    (s0..s4)
    QS_GATE1 = 1,     // s5 = q_m a b + q_l a + q_r b                                   (s5 = q_m, s6 = q_l, s7 = q_r)
    QS_GATE2 = 2,     // s5 += q_o c + q_4 d                                            (s6 = q_o, s7 = q_4)
    QS_GATE3 = 3,     // t  += q_arith (s5 + q_c)                                       (s6 = q_c, s7 = q_arith)
    QS_PERM1 = 4,     // t  += PI (if any);  s6 = (a + beta sigma_1 + gamma)(b + beta sigma_2 + gamma)   (s5 = PI, s6, s7 = sigma_1, _2)
    QS_PERM2 = 5,     // t  = (t - alpha s6 (c + beta sigma_3 + gamma)(d + beta sigma_4 + gamma) z(omega x)) c_j^-1   (s5, s7 = sigma_3, _4)
    QS_BLIND = 6,     // (pg_quotient_blinded only, before QS_PERM_NUM; quotient_blind_kernel)  s0..s4 += x^n tail(x)
};

struct QuotientChunk {
    uint4 *t;             // chunk j of d_t: n points
    uint4 *s;             // scratch: column c at s + 2 c n
    uint64_t n;
    uint32_t has_pi;
    NttTable x;           // x = g_j omega^i
    Fr alpha, beta, gamma;
    Fr beta_k[4];         // beta k_j
    Fr n_fr;              // n as a field element
    Fr alpha2_c;          // alpha^2 c_j
    Fr c_inv;             // c_j^-1
    // QS_BLIND alone reads these (pg_quotient leaves them zero)
    const uint4 *tail[5]; // rows n.. of the caller's a, b, c, d (two rows each) and z (three)
    Fr xn;                // x^n = c_j + 1 on the chunk
};

__device__ __forceinline__ Fr q_col(const QuotientChunk &A, uint32_t c, uint64_t i) { return pp_load(A.s, c * A.n + i); }

// one of QS_GATE1 .. QS_PERM2 (see the enum) at point i
template <int OP>
__device__ __forceinline__ void quotient_point(const QuotientChunk &A, uint64_t i) {
    if (OP == QS_GATE1) {
        const Fr a = q_col(A, 0, i), b = q_col(A, 1, i);
        const Fr ab = fr_mul(fr_add(fr_mul(q_col(A, 5, i), a), q_col(A, 7, i)), b);  // (q_m a + q_r) b
        pp_store(A.s, 5 * A.n + i, fr_add(ab, fr_mul(q_col(A, 6, i), a)));
    } else if (OP == QS_GATE2) {
        const Fr g = fr_add(fr_mul(q_col(A, 6, i), q_col(A, 2, i)), fr_mul(q_col(A, 7, i), q_col(A, 3, i)));
        pp_store(A.s, 5 * A.n + i, fr_add(q_col(A, 5, i), g));
    } else if (OP == QS_GATE3) {
        const Fr g = fr_mul(q_col(A, 7, i), fr_add(q_col(A, 5, i), q_col(A, 6, i)));
        pp_store(A.t, i, fr_add(pp_load(A.t, i), g));
    } else if (OP == QS_PERM1) {
        if (A.has_pi) pp_store(A.t, i, fr_add(pp_load(A.t, i), q_col(A, 5, i)));
        const Fr f0 = fr_add(fr_add(q_col(A, 0, i), fr_mul(A.beta, q_col(A, 6, i))), A.gamma);
        const Fr f1 = fr_add(fr_add(q_col(A, 1, i), fr_mul(A.beta, q_col(A, 7, i))), A.gamma);
        pp_store(A.s, 6 * A.n + i, fr_mul(f0, f1));
    } else if (OP == QS_PERM2) {
        const Fr f2 = fr_add(fr_add(q_col(A, 2, i), fr_mul(A.beta, q_col(A, 5, i))), A.gamma);
        const Fr f3 = fr_add(fr_add(q_col(A, 3, i), fr_mul(A.beta, q_col(A, 7, i))), A.gamma);
        const Fr zw = q_col(A, 4, (i + 1) & (A.n - 1));
        const Fr den = fr_mul(fr_mul(fr_mul(q_col(A, 6, i), f2), fr_mul(f3, zw)), A.alpha);
        pp_store(A.t, i, fr_mul(fr_sub(pp_load(A.t, i), den), A.c_inv));
    }
}

template <int OP>
__global__ __launch_bounds__(kThreads) void quotient_step_kernel(const QuotientChunk A) {
    if (OP != QS_PERM_NUM) {
        for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < A.n; i += (uint64_t)gridDim.x * kThreads)
            quotient_point<OP>(A, i);
        return;
    }
    // QS_PERM_NUM: a tile of kQTile points per workgroup step, lane t taking points t, t + 256, ... of it
    const uint32_t t = threadIdx.x;
    const uint64_t tiles = (A.n + kQTile - 1) / kQTile;
#pragma unroll 1
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t base = tile * kQTile;
        Fr P = fr_one();  // running product of d_k = n (x_k - 1)
#pragma unroll 1
        for (uint32_t k = 0; k < kQRowsPerLane; k++) {
            const uint64_t i = base + (uint64_t)k * kThreads + t;
            if (i >= A.n) break;
            const Fr d = fr_sub(fr_mul(A.n_fr, ntt_pow(A.x, i)), A.n_fr);
            pp_store(A.t, i, P);  // P_{k-1}
            P = fr_mul(P, d);
        }
        Fr I = fr_invert_or_zero(P);  // 1 / P_last
#pragma unroll 1
        for (int k = (int)kQRowsPerLane - 1; k >= 0; k--) {
            const uint64_t i = base + (uint64_t)k * kThreads + t;
            if (i >= A.n) continue;
            const Fr x = ntt_pow(A.x, i);
            const Fr d = fr_sub(fr_mul(A.n_fr, x), A.n_fr);
            const Fr inv = fr_mul(I, pp_load(A.t, i));  // 1 / d_k = P_{k-1} / P_k
            I = fr_mul(I, d);                            // 1 / P_{k-1}
            const Fr z = q_col(A, 4, i);
            Fr num = z;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) num = fr_mul(num, fr_add(fr_add(q_col(A, j, i), fr_mul(A.beta_k[j], x)), A.gamma));
            const Fr l1 = fr_mul(fr_mul(fr_sub(z, fr_one()), inv), A.alpha2_c);
            pp_store(A.t, i, fr_add(fr_mul(num, A.alpha), l1));
        }
    }
}

// QS_BLIND: s_j[i] += x^n (h1 x + h0) for the wires (j < 4) and s_4[i] += x^n ((h2 x + h1) x + h0) for z, h = the tail rows, which
// every lane reads once and multiplies by x^n
__global__ __launch_bounds__(kThreads) void quotient_blind_kernel(const QuotientChunk A) {
    Fr h[4][2], hz[3];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        h[j][0] = fr_mul(A.xn, pp_load(A.tail[j], 0));
        h[j][1] = fr_mul(A.xn, pp_load(A.tail[j], 1));
    }
#pragma unroll
    for (uint32_t r = 0; r < 3; r++) hz[r] = fr_mul(A.xn, pp_load(A.tail[4], r));
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < A.n; i += (uint64_t)gridDim.x * kThreads) {
        const Fr x = ntt_pow(A.x, i);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            pp_store(A.s, j * A.n + i, fr_add(q_col(A, j, i), fr_add(fr_mul(h[j][1], x), h[j][0])));
        const Fr tz = fr_add(fr_mul(fr_add(fr_mul(hz[2], x), hz[1]), x), hz[0]);
        pp_store(A.s, 4 * A.n + i, fr_add(q_col(A, 4, i), tz));
    }
}

// the inverse 4-point DFT across the chunks, per k0 < n, in place: r_j = t[j n + k0] -> t[k0 + n k1] = scale[k1] sum_j iota^(j k1) r_j,
// iota = zeta^-n (iota^2 = -1), scale[k1] = 4^-1 g^(-n k1)
struct QuotientCombine {
    uint4 *t;
    uint64_t n;
    Fr iota;
    Fr scale[4];
};
__global__ __launch_bounds__(kThreads) void quotient_combine_kernel(const QuotientCombine A) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < A.n; i += (uint64_t)gridDim.x * kThreads) {
        const Fr r0 = pp_load(A.t, i), r1 = pp_load(A.t, A.n + i), r2 = pp_load(A.t, 2 * A.n + i), r3 = pp_load(A.t, 3 * A.n + i);
        const Fr e0 = fr_add(r0, r2), e1 = fr_sub(r0, r2), o0 = fr_add(r1, r3), o1 = fr_mul(A.iota, fr_sub(r1, r3));
        pp_store(A.t, i, fr_mul(fr_add(e0, o0), A.scale[0]));
        pp_store(A.t, A.n + i, fr_mul(fr_add(e1, o1), A.scale[1]));
        pp_store(A.t, 2 * A.n + i, fr_mul(fr_sub(e0, o0), A.scale[2]));
        pp_store(A.t, 3 * A.n + i, fr_mul(fr_sub(e1, o1), A.scale[3]));
    }
}

// the seven coefficients of the blinded quotient that 4n points cannot hold.  A factor is its top seven coefficients, highest
// first (f[d] = the coefficient d below its degree); a product's top seven are then p[d] = sum_{d1 <= d} a[d1] b[d - d1].
constexpr uint32_t kQTop = 7;
constexpr uint32_t kQTopLanes = 64;  // one wave; lane 0 works
struct QuotientTop {
    const uint4 *w[4], *sigma[4], *z;  // the caller's inputs: n + 2, n and n + 3 rows
    uint4 *t;                          // 4n + 8 rows
    uint64_t n;
    Fr alpha, beta, g4n;               // g4n = g^(4n)
    Fr zw[kQTop];                      // omega^(n + 2 - d): z(omega X)'s coefficient d below the top is z's times this
};

// acc = the top seven of acc * b, in place: p[d] needs acc[0..d] only, so d runs downwards
__device__ __forceinline__ void quotient_top_mul(Fr (&acc)[kQTop], const Fr (&b)[kQTop]) {
#pragma unroll
    for (int d = (int)kQTop - 1; d >= 0; d--) {
        Fr p = fr_mul(acc[0], b[d]);
#pragma unroll
        for (int d1 = 1; d1 <= d; d1++) p = fr_add(p, fr_mul(acc[d1], b[d - d1]));
        acc[d] = p;
    }
}

// one working lane.  First T_i = N[5n + i] = alpha (P[6 - i] - P'[6 - i]) into t[4n + i], P = the top of z prod_j w_j (side 0)
// and P' = the top of z(omega X) prod_j (w_j + beta sigma_j) (side 1); then t[k] -= g^(4n) T_k.  It runs after the combine.
__global__ __launch_bounds__(kQTopLanes) void quotient_top_kernel(const QuotientTop A) {
    if (blockIdx.x | threadIdx.x) return;
    const uint64_t n = A.n;
#pragma unroll 1
    for (uint32_t side = 0; side < 2; side++) {
        Fr acc[kQTop];
#pragma unroll
        for (uint32_t d = 0; d < kQTop; d++) {
            acc[d] = pp_load(A.z, n + 2 - d);
            if (side) acc[d] = fr_mul(acc[d], A.zw[d]);
        }
#pragma unroll 1
        for (uint32_t j = 0; j < 4; j++) {
            const uint4 *w = A.w[j], *sg = A.sigma[j];
            Fr b[kQTop];
#pragma unroll
            for (uint32_t d = 0; d < kQTop; d++) {
                b[d] = pp_load(w, n + 1 - d);
                if (side && d >= 2) b[d] = fr_add(b[d], fr_mul(A.beta, pp_load(sg, n + 1 - d)));
            }
            quotient_top_mul(acc, b);
        }
#pragma unroll
        for (uint32_t d = 0; d < kQTop; d++) {
            const uint64_t row = 4 * n + (kQTop - 1 - d);
            const Fr v = fr_mul(A.alpha, acc[d]);
            pp_store(A.t, row, side ? fr_sub(pp_load(A.t, row), v) : v);
        }
    }
    pp_store(A.t, 4 * n + kQTop, fr_zero());
#pragma unroll 1
    for (uint32_t k = 0; k < kQTop; k++) pp_store(A.t, k, fr_sub(pp_load(A.t, k), fr_mul(A.g4n, pp_load(A.t, 4 * n + k))));
}

// ---- the range widget's term (pg_quotient_range) ------------------------------------------------------------
//   N(x) += q_range(x) [ alpha^3 delta(b - 4a) + alpha^4 delta(c - 4b) + alpha^5 delta(a(omega x) - 4c) ],  delta(f) = f (f-1)(f-2)(f-3)
// a, b and c are resident in scratch columns 0..2 (blinded already, when the call is), a(omega x) is entry (i + 1) mod n of column 0 as
// z(omega x) is of column 4, and q_range has just been transformed into column 5.  The step runs after QS_GATE3 and before QS_PERM1
// (which reuses column 5): t is still N's partial sum, not yet divided by c_j.
struct QuotientRange {
    Fr alpha[3];  // alpha^3, alpha^4, alpha^5
};
__device__ __forceinline__ Fr range_delta(const Fr &hi, const Fr &lo) {  // delta(hi - 4 lo)
    const Fr two = fr_add(lo, lo), f = fr_sub(hi, fr_add(two, two)), one = fr_one();
    const Fr f1 = fr_sub(f, one), f2 = fr_sub(f1, one), f3 = fr_sub(f2, one);
    return fr_mul(fr_mul(f, f1), fr_mul(f2, f3));
}
__global__ __launch_bounds__(kThreads) void quotient_range_kernel(const QuotientChunk A, const QuotientRange G) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < A.n; i += (uint64_t)gridDim.x * kThreads) {
        const Fr a = q_col(A, 0, i), b = q_col(A, 1, i), c = q_col(A, 2, i), aw = q_col(A, 0, (i + 1) & (A.n - 1));
        Fr s = fr_mul(G.alpha[0], range_delta(b, a));
        s = fr_add(s, fr_mul(G.alpha[1], range_delta(c, b)));
        s = fr_add(s, fr_mul(G.alpha[2], range_delta(aw, c)));
        pp_store(A.t, i, fr_add(pp_load(A.t, i), fr_mul(q_col(A, 5, i), s)));
    }
}

// Blinded: the term has degree <= (n - 1) + 4 (n + 1) = 5n + 3, so it adds to T_0 .. T_3: the truncated product of the top four
// coefficients of q_range (rows n-1 .. n-4) and of the four factors of each delta, which share theirs (rows n+1 .. n-2 of hi - 4 lo,
// times omega^row for a(omega X); the constants 1, 2, 3 lie in row 0, below the windows for n >= 8).  One working lane, after
// quotient_top_kernel, whose correction is linear: t[4n + i] += X_i and t[i] -= g^(4n) X_i.
constexpr uint32_t kQRangeTop = 4;
struct QuotientRangeTop {
    const uint4 *w[3], *q_range;  // the caller's a, b, c (n + 2 rows) and q_range (n rows)
    uint4 *t;                     // 4n + 8 rows
    uint64_t n;
    Fr alpha[3], g4n;
    Fr aw[kQRangeTop];            // omega^(n + 1 - d): a(omega X)'s coefficient d below the top is a's times this
};
__device__ __forceinline__ void quotient_range_top_mul(Fr (&acc)[kQRangeTop], const Fr (&b)[kQRangeTop]) {
#pragma unroll
    for (int d = (int)kQRangeTop - 1; d >= 0; d--) {
        Fr p = fr_mul(acc[0], b[d]);
#pragma unroll
        for (int d1 = 1; d1 <= d; d1++) p = fr_add(p, fr_mul(acc[d1], b[d - d1]));
        acc[d] = p;
    }
}
__global__ __launch_bounds__(kQTopLanes) void quotient_range_top_kernel(const QuotientRangeTop A) {
    if (blockIdx.x | threadIdx.x) return;
    const uint64_t n = A.n;
    Fr q[kQRangeTop], X[kQRangeTop];
#pragma unroll
    for (uint32_t d = 0; d < kQRangeTop; d++) {
        q[d] = pp_load(A.q_range, n - 1 - d);
        X[d] = fr_zero();
    }
#pragma unroll 1
    for (uint32_t s = 0; s < 3; s++) {
        const uint4 *lo = A.w[s], *hi = A.w[s == 2 ? 0 : s + 1];
        Fr f[kQRangeTop], acc[kQRangeTop];
#pragma unroll
        for (uint32_t d = 0; d < kQRangeTop; d++) {
            Fr h = pp_load(hi, n + 1 - d);
            if (s == 2) h = fr_mul(h, A.aw[d]);
            const Fr l = pp_load(lo, n + 1 - d), two = fr_add(l, l);
            f[d] = fr_sub(h, fr_add(two, two));
            acc[d] = f[d];
        }
#pragma unroll 1
        for (uint32_t k = 0; k < 3; k++) quotient_range_top_mul(acc, f);
        quotient_range_top_mul(acc, q);
#pragma unroll
        for (uint32_t d = 0; d < kQRangeTop; d++) X[d] = fr_add(X[d], fr_mul(A.alpha[s], acc[d]));
    }
#pragma unroll
    for (uint32_t d = 0; d < kQRangeTop; d++) {
        const uint64_t i = kQRangeTop - 1 - d;  // acc[d] = the coefficient 5n + 3 - d
        pp_store(A.t, 4 * n + i, fr_add(pp_load(A.t, 4 * n + i), X[d]));
        pp_store(A.t, i, fr_sub(pp_load(A.t, i), fr_mul(A.g4n, X[d])));
    }
}

// ---- evaluation at a point ----------------------------------------------------------------------------------------------------
struct PolyEval {
    const uint4 *c;          // column j at c + 2 j stride
    uint64_t n_cols, stride, n, segs;  // segs = ceil(n / kEvalSeg)
    Fr x256;                 // x^256
    const uint4 *x_lane;     // x^t, t < 256
    const uint4 *x_seg;      // x^(s kEvalSeg), s < segs
    uint4 *partial;          // n_cols x segs
    uint4 *out;              // n_cols
};

// the sum of the 256 lanes' x (every lane calls it; lane 0 gets the sum); buf: 256 entries of LDS
__device__ __forceinline__ Fr eval_block_sum(const Fr &x, FrVec *buf) {
    const uint32_t t = threadIdx.x;
    buf[t].f = x;
    __syncthreads();
#pragma unroll
    for (uint32_t h = kThreads / 2; h > 0; h >>= 1) {
        if (t < h) buf[t].f = fr_add(buf[t].f, buf[t + h].f);
        __syncthreads();
    }
    const Fr r = buf[0].f;
    __syncthreads();  // (buf is reused)
    return r;
}

__global__ __launch_bounds__(kThreads) void poly_eval_kernel(const PolyEval A) {
    __shared__ FrVec buf[kThreads];
    const uint32_t t = threadIdx.x;
    const Fr xt = pp_load(A.x_lane, t);
    const uint64_t items = A.n_cols * A.segs;
#pragma unroll 1
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const uint64_t col = it / A.segs, seg = it - col * A.segs, first = seg * kEvalSeg;
        const uint4 *c = A.c + 2 * col * A.stride;
        Fr acc = fr_zero();
#pragma unroll 4
        for (int k = (int)kEvalPerLane - 1; k >= 0; k--) {
            const uint64_t i = first + (uint64_t)k * kThreads + t;
            acc = fr_add(fr_mul(acc, A.x256), i < A.n ? pp_load(c, i) : fr_zero());
        }
        const Fr sum = eval_block_sum(fr_mul(acc, xt), buf);
        if (t == 0) pp_store(A.partial, it, fr_mul(sum, pp_load(A.x_seg, seg)));
    }
}

// one column per workgroup step
__global__ __launch_bounds__(kThreads) void poly_eval_reduce_kernel(const PolyEval A) {
    __shared__ FrVec buf[kThreads];
#pragma unroll 1
    for (uint64_t col = blockIdx.x; col < A.n_cols; col += gridDim.x) {
        Fr acc = fr_zero();
        for (uint64_t s = threadIdx.x; s < A.segs; s += kThreads) acc = fr_add(acc, pp_load(A.partial, col * A.segs + s));
        const Fr sum = eval_block_sum(acc, buf);
        if (threadIdx.x == 0) pp_store(A.out, col, sum);
    }
}

}  // namespace pg
