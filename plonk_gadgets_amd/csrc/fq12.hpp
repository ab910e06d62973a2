// fq12.hpp -- Fq12 for the BLS12-381 pairing (pairing.hpp), in the DIRECT SEXTIC form: six Fq2 coefficients over w^0 .. w^5 with
// w^6 = XI = 1 + u.  (The tower Fq6 = Fq2[v] / (v^3 - XI), Fq12 = Fq6[w] / (w^2 - v) is the same field with v = w^2: the even
// coefficients are the Fq6 part A, the odd ones B of A + B w; only the inversion below uses that view.)
//
// An element is 144 registers, so no lane ever holds one: an element lives in memory (LDS in the
// kernel, the stack on the host) as Fq2[6], and the functions here compute ONE coefficient of a result from operands in
// memory -- the unit of work of one of the six lanes that share a pairing.  Loops over fq2_mul stay rolled on the device.
// One source for host and gfx950 device code; tests/pairing_model.py is the Python model of every function.
#pragma once

#include "fq2.hpp"
#include "pairing_constants.inc"

namespace pg {

struct Fq12 {
    Fq2 c[6];
};

#if defined(__HIPCC__)
static __device__ __constant__ const uint64_t kGamma1Dev[6][12] = PG_GAMMA1_TABLE;
static __device__ __constant__ const uint64_t kGamma2Dev[6][6] = PG_GAMMA2_TABLE;
#endif
static const uint64_t kGamma1Host[6][12] = PG_GAMMA1_TABLE;
static const uint64_t kGamma2Host[6][6] = PG_GAMMA2_TABLE;

// XI^(k (p - 1) / 6)
PG_HD Fq2 fq12_gamma1(int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t *t = kGamma1Dev[k];
#else
    const uint64_t *t = kGamma1Host[k];
#endif
    return Fq2{Fq{{t[0], t[1], t[2], t[3], t[4], t[5]}}, Fq{{t[6], t[7], t[8], t[9], t[10], t[11]}}};
}
// XI^(k (p^2 - 1) / 6), an element of Fq
PG_HD Fq fq12_gamma2(int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t *t = kGamma2Dev[k];
#else
    const uint64_t *t = kGamma2Host[k];
#endif
    return Fq{{t[0], t[1], t[2], t[3], t[4], t[5]}};
}

// coefficient k of 1
PG_HD Fq2 fq12_one_coeff(int k) { return k == 0 ? fq2_one() : fq2_zero(); }

// coefficient k of a b: sum_{i + j = k} a_i b_j + XI sum_{i + j = k + 6} a_i b_j -- six Fq2 products (18 Fq products)
PG_HD Fq2 fq12_mul_coeff(const Fq2 *a, const Fq2 *b, int k) {
    Fq2 lo = fq2_zero(), hi = fq2_zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 6; i++) {
        const int j = k - i;
        const Fq2 t = fq2_mul(a[i], b[j < 0 ? j + 6 : j]);
        // (selects, not a branch: the six lanes of a pairing sit in one wave with different k)
        lo = fq2_add(lo, j < 0 ? fq2_zero() : t);
        hi = fq2_add(hi, j < 0 ? t : fq2_zero());
    }
    return fq2_add(lo, fq2_mul_xi(hi));
}

// coefficient k of f (l0 + l2 w^2 + l3 w^3), l0 and l2 in Fq2, l3 in Fq: the product by a line of the Miller loop -- two Fq2
// products and one by an Fq element (8 Fq products)
PG_HD Fq2 fq12_sparse_coeff(const Fq2 *f, const Fq2 &l0, const Fq2 &l2, const Fq &l3, int k) {
    const Fq2 t2 = fq2_mul(f[k < 2 ? k + 4 : k - 2], l2);
    const Fq2 t3 = fq2_mul_fq(f[k < 3 ? k + 3 : k - 3], l3);
    const Fq2 z = fq2_zero();
    const Fq2 hi = fq2_add(k < 2 ? t2 : z, k < 3 ? t3 : z), lo = fq2_add(k < 2 ? z : t2, k < 3 ? z : t3);
    return fq2_add(fq2_add(fq2_mul(f[k], l0), lo), fq2_mul_xi(hi));
}

// coefficient k of a^(p^6) (w -> -w), given a's coefficient k: the inverse of an element of norm 1 over Fq6
PG_HD Fq2 fq12_conj_coeff(const Fq2 &c, int k) { return (k & 1) ? fq2_neg(c) : c; }
// coefficient k of a^p: conj(c) XI^(k (p - 1) / 6)
PG_HD Fq2 fq12_frobenius_coeff(const Fq2 &c, int k) { return fq2_mul(fq2_conj(c), fq12_gamma1(k)); }
// coefficient k of a^(p^2): c XI^(k (p^2 - 1) / 6)
PG_HD Fq2 fq12_frobenius2_coeff(const Fq2 &c, int k) { return fq2_mul_fq(c, fq12_gamma2(k)); }

// ---- the tower view, for the inversion: an Fq6 element's coefficient j lies at x[j * stride] ----------------------------------
// o = a b over v^3 = XI; o is contiguous and distinct from a and b
PG_HD void fq6_mul(Fq2 *o, const Fq2 *a, int sa, const Fq2 *b, int sb) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int k = 0; k < 3; k++) {
        Fq2 lo = fq2_zero(), hi = fq2_zero();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int i = 0; i < 3; i++) {
            const int j = k - i;
            const Fq2 t = fq2_mul(a[i * sa], b[(j < 0 ? j + 3 : j) * sb]);
            lo = fq2_add(lo, j < 0 ? fq2_zero() : t);
            hi = fq2_add(hi, j < 0 ? t : fq2_zero());
        }
        o[k] = fq2_add(lo, fq2_mul_xi(hi));
    }
}

// o = 1 / a in Fq6 (contiguous, o distinct from a); 0 for 0
PG_HD void fq6_inverse(Fq2 *o, const Fq2 *a) {
    // (the t_j are parked in o, and every operand is read again where it is used: few values are live at once)
    o[0] = fq2_sub(fq2_square(a[0]), fq2_mul_xi(fq2_mul(a[1], a[2])));
    o[1] = fq2_sub(fq2_mul_xi(fq2_square(a[2])), fq2_mul(a[0], a[1]));
    o[2] = fq2_sub(fq2_square(a[1]), fq2_mul(a[0], a[2]));
    const Fq2 d = fq2_add(fq2_mul(a[0], o[0]), fq2_mul_xi(fq2_add(fq2_mul(a[2], o[1]), fq2_mul(a[1], o[2]))));
    const Fq2 di = fq2_inverse(d);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int j = 0; j < 3; j++) o[j] = fq2_mul(o[j], di);
}

// out = 1 / a (0 for 0), by ONE thread: (A + B w)^-1 = (A - B w) / (A^2 - v B^2).  tmp: 12 Fq2 of workspace, distinct from a and
// out; out may be a.
PG_HD void fq12_inverse(const Fq2 *a, Fq2 *out, Fq2 *tmp) {
    Fq2 *aa = tmp, *bb = tmp + 3, *d = tmp + 6, *di = tmp + 9;
    fq6_mul(aa, a, 2, a, 2);
    fq6_mul(bb, a + 1, 2, a + 1, 2);
    d[0] = fq2_sub(aa[0], fq2_mul_xi(bb[2]));
    d[1] = fq2_sub(aa[1], bb[0]);
    d[2] = fq2_sub(aa[2], bb[1]);
    fq6_inverse(di, d);
    fq6_mul(aa, a, 2, di, 1);
    fq6_mul(bb, a + 1, 2, di, 1);
    for (int j = 0; j < 3; j++) {
        out[2 * j] = aa[j];
        out[2 * j + 1] = fq2_neg(bb[j]);
    }
}

// ---- whole elements, one thread (the host's forms; the kernel spreads the coefficient functions over six lanes) ------------------------
PG_HD Fq12 fq12_one() {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq12_one_coeff(k);
    return r;
}
PG_HD bool fq12_eq(const Fq12 &a, const Fq12 &b) {
    bool e = true;
    for (int k = 0; k < 6; k++) e = e && fq2_eq(a.c[k], b.c[k]);
    return e;
}
PG_HD Fq12 fq12_mul(const Fq12 &a, const Fq12 &b) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq12_mul_coeff(a.c, b.c, k);
    return r;
}
PG_HD Fq12 fq12_square(const Fq12 &a) { return fq12_mul(a, a); }
PG_HD Fq12 fq12_mul_sparse(const Fq12 &f, const Fq2 &l0, const Fq2 &l2, const Fq &l3) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq12_sparse_coeff(f.c, l0, l2, l3, k);
    return r;
}
PG_HD Fq12 fq12_add(const Fq12 &a, const Fq12 &b) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq2_add(a.c[k], b.c[k]);
    return r;
}
PG_HD Fq12 fq12_sub(const Fq12 &a, const Fq12 &b) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq2_sub(a.c[k], b.c[k]);
    return r;
}
PG_HD Fq12 fq12_neg(const Fq12 &a) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq2_neg(a.c[k]);
    return r;
}
PG_HD Fq12 fq12_conj(const Fq12 &a) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq12_conj_coeff(a.c[k], k);
    return r;
}
PG_HD Fq12 fq12_frobenius(const Fq12 &a) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq12_frobenius_coeff(a.c[k], k);
    return r;
}
PG_HD Fq12 fq12_frobenius2(const Fq12 &a) {
    Fq12 r;
    for (int k = 0; k < 6; k++) r.c[k] = fq12_frobenius2_coeff(a.c[k], k);
    return r;
}
PG_HD Fq12 fq12_invert(const Fq12 &a) {
    Fq12 r;
    Fq2 tmp[12];
    fq12_inverse(a.c, r.c, tmp);
    return r;
}

}  // namespace pg
