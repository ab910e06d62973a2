// pairing.hpp -- the BLS12-381 pairing check: d_ok[i] = (prod_j e(P_ij, Q_j) == 1) for prepared Q_j (g2.hpp).  DESIGN section 3.13.
//
// An Fq12 element is 144 registers, a product needs three of them live: one lane per pairing cannot fit the 512 registers a
// lane can have, and scratch is ruled out.  So SIX lanes share a check: f and three temporaries live in LDS as Fq2[6] each
// (2 304 bytes per check), lane k computes coefficient k of every product (fq12.hpp: six Fq2 products, or the three of a line
// product) into registers, the workgroup meets at a barrier, the lanes store, and it meets again.  A workgroup of 252 lanes
// (four waves: the kernel needs more than 256 registers, so a SIMD holds one wave and a CU one workgroup) carries 42 checks in
// 94.5 KiB of LDS.  Every lane of the workgroup runs the same straight sequence of operations (the bits
// of |x| are constants), so every barrier is reached by all; a workgroup's spare checks recompute its last real one and write
// nothing.  Nothing waits on another workgroup.
//
// Per check: the Miller loop over the 68 prepared lines (63 squarings; per line and pair one sparse product, all pairs
// accumulated into one f), a conjugation (x < 0), then ONE final exponentiation: the easy part f^((p^6 - 1)(p^2 + 1)) with an
// inversion done by the check's lane 0 through the tower view, and the hard part by
//     3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3        (Hayashida, Hayasaka and Teruya, 2020),
// five powers by |x| of 63 squarings and 5 products each.  So the GT value is e(P, Q)^3 -- the CUBE of the plain power
// (p^12 - 1) / r; 3 is coprime to r, so it is 1 exactly when the pairing product is.  Squarings are plain products (no cyclotomic
// squaring yet).  pairing_host below is the same sequence on one host thread: what tests/cpp/pairing_host.cpp compares with
// tests/pairing_model.py, and what the kernel is compared with in turn.
#pragma once

#include "g1.hpp"
#include "g2.hpp"

namespace pg {

constexpr int kPairLanes = 6;       // lanes per check
constexpr int kPairChecks = 42;     // checks per workgroup: 252 lanes, four waves -- one per SIMD, all a CU holds at > 256 registers
constexpr int kPairThreads = kPairLanes * kPairChecks;
constexpr int kPairMaxPairs = 8;    // the points of a check are staged in two LDS slots: 12 Fq2 = 12 x 96 bytes hold up to 12 points
constexpr int kPairSlots = 4;

// ---- one host thread ------------------------------------------------------------------------------------------------------
// the Miller value of prod_j (P_j, lines_j), conjugated
inline Fq12 pairing_host_miller(const G1A *pts, const G2Line *const *lines, int n_pairs) {
    Fq12 f = fq12_one();
    int idx = 0;
    for (int b = 62; b >= 0; b--) {
        f = fq12_square(f);
        for (int l = 0; l < 1 + (int)((kAteLoop >> b) & 1); l++, idx++)
            for (int j = 0; j < n_pairs; j++) {
                if (g1a_is_identity(pts[j])) continue;
                const G2Line &ln = lines[j][idx];
                f = fq12_mul_sparse(f, ln.c0, fq2_mul_fq(ln.c2, pts[j].x), pts[j].y);
            }
    }
    return fq12_conj(f);
}

inline Fq12 pairing_host_pow_x_abs(const Fq12 &a) {
    Fq12 r = a;
    for (int b = 62; b >= 0; b--) {
        r = fq12_square(r);
        if ((kAteLoop >> b) & 1) r = fq12_mul(r, a);
    }
    return r;
}

// f^(3 (p^12 - 1) / r)
inline Fq12 pairing_host_final_exp(const Fq12 &f) {
    Fq12 t = fq12_mul(fq12_conj(f), fq12_invert(f));
    const Fq12 m = fq12_mul(fq12_frobenius2(t), t);
    t = fq12_conj(fq12_mul(pairing_host_pow_x_abs(m), m));                           // m^(x - 1)
    t = fq12_conj(fq12_mul(pairing_host_pow_x_abs(t), t));                           // ^(x - 1)
    t = fq12_mul(fq12_conj(pairing_host_pow_x_abs(t)), fq12_frobenius(t));           // ^(x + p)
    const Fq12 a = pairing_host_pow_x_abs(pairing_host_pow_x_abs(t));                // ^(x^2)
    t = fq12_mul(fq12_mul(a, fq12_frobenius2(t)), fq12_conj(t));                     // ^(x^2 + p^2 - 1)
    return fq12_mul(t, fq12_mul(fq12_square(m), m));
}

#if defined(__HIPCC__)
// the lines of up to kPairMaxPairs prepared points (device pointers, kAteLines G2Lines each)
struct PairingLines {
    const G2Line *q[kPairMaxPairs];
};

// points: [n_checks][n_pairs]; ok: [n_checks] or NULL; gt: [n_checks][6] Fq2 or NULL
__global__ __launch_bounds__(kPairThreads) void pairing_check_kernel(const G1A *__restrict__ points, PairingLines L, uint64_t n_checks,
                                                                     uint32_t n_pairs, uint8_t *__restrict__ ok, Fq2 *__restrict__ gt) {
    __shared__ Fq2 sh[kPairChecks][kPairSlots][6];
    __shared__ uint32_t differs[kPairChecks];
    const int c = threadIdx.x / kPairLanes, k = threadIdx.x % kPairLanes;
    uint64_t check = (uint64_t)blockIdx.x * kPairChecks + c;
    const bool live = check < n_checks;
    if (!live) check = n_checks - 1;
    Fq2 *F = sh[c][0], *T = sh[c][1], *A = sh[c][2], *B = sh[c][3];
    G1A *pts = reinterpret_cast<G1A *>(T);  // (T and A, contiguous: free until the final exponentiation)
    for (uint32_t j = k; j < n_pairs; j += kPairLanes) pts[j] = points[check * n_pairs + j];
    F[k] = fq12_one_coeff(k);
    if (k == 0) differs[c] = 0;
    __syncthreads();

    // o = a b; o may be a or b: every lane holds its coefficient until all have read
    auto mul = [=](Fq2 *o, const Fq2 *a, const Fq2 *b) {
        const Fq2 r = fq12_mul_coeff(a, b, k);
        __syncthreads();
        o[k] = r;
        __syncthreads();
    };
    // A = base^|x|
    auto pow_x_abs = [=](const Fq2 *base) {
        A[k] = base[k];
        __syncthreads();
#pragma unroll 1
        for (int b = 62; b >= 0; b--) {
            mul(A, A, A);
            if ((kAteLoop >> b) & 1) mul(A, A, base);
        }
    };

    // ---- the Miller loop
    uint32_t idx = 0;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        mul(F, F, F);
        const uint32_t nl = 1 + (uint32_t)((kAteLoop >> b) & 1);
#pragma unroll 1
        for (uint32_t l = 0; l < nl; l++, idx++) {
#pragma unroll 1
            for (uint32_t j = 0; j < n_pairs; j++) {
                const G2Line *q = L.q[0];
#pragma unroll
                for (uint32_t jj = 1; jj < kPairMaxPairs; jj++) q = j == jj ? L.q[jj] : q;
                const G2Line ln = q[idx];
                const G1A p = pts[j];
                const Fq2 r = g1a_is_identity(p) ? F[k] : fq12_sparse_coeff(F, ln.c0, fq2_mul_fq(ln.c2, p.x), p.y, k);
                __syncthreads();
                F[k] = r;
                __syncthreads();
            }
        }
    }

    F[k] = fq12_conj_coeff(F[k], k);  // x < 0
    __syncthreads();

    // ---- the easy part: m = (conj(f) / f)^(p^2 + 1), left in F
    if (k == 0) fq12_inverse(F, B, T);  // (T and A as its 12 Fq2 of workspace; the points are no longer needed)
    __syncthreads();
    F[k] = fq12_conj_coeff(F[k], k);
    __syncthreads();
    mul(T, F, B);
    B[k] = fq12_frobenius2_coeff(T[k], k);
    __syncthreads();
    mul(F, B, T);
    const Fq2 *M = F;

    // ---- the hard part, left in T
    pow_x_abs(M);
    mul(T, A, M);
    T[k] = fq12_conj_coeff(T[k], k);  // m^(x - 1)
    __syncthreads();
    pow_x_abs(T);
    mul(T, A, T);
    T[k] = fq12_conj_coeff(T[k], k);  // ^(x - 1)
    __syncthreads();
    pow_x_abs(T);
    A[k] = fq12_conj_coeff(A[k], k);
    B[k] = fq12_frobenius_coeff(T[k], k);
    __syncthreads();
    mul(T, A, B);                      // ^(x + p)
    pow_x_abs(T);
    B[k] = A[k];
    __syncthreads();
    pow_x_abs(B);                      // ^(x^2)
    B[k] = fq12_frobenius2_coeff(T[k], k);
    __syncthreads();
    mul(A, A, B);
    T[k] = fq12_conj_coeff(T[k], k);
    __syncthreads();
    mul(T, A, T);                      // ^(x^2 + p^2 - 1)
    mul(A, M, M);
    mul(A, A, M);
    mul(T, T, A);

    const Fq2 v = T[k];
    if (!fq2_eq(v, fq12_one_coeff(k))) atomicOr(&differs[c], 1u);
    __syncthreads();
    if (live) {
        if (gt) gt[check * 6 + k] = v;
        if (ok && k == 0) ok[check] = differs[c] ? 0 : 1;
    }
}
#endif  // __HIPCC__

}  // namespace pg
