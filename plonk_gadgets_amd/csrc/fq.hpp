// fq.hpp -- BLS12-381 base field Fq for the engine's G1 arithmetic (g1.hpp, msm.hpp): 6 x 64-bit limbs, Montgomery
// form x*R mod p with R = 2^384, values always fully reduced in [0, p) so that equal field elements have identical limbs
// (the invariant fr.hpp keeps, and the one the limb-for-limb tests rely on).  One source for host and gfx950 device code.
//
// Device forms: the product works on 12 x 32-bit words around v_mad_u64_u32 (fq_mul below).  Unlike fr.hpp's products it is
// plain C++: p is not 1 mod 2^32, so every quotient digit costs a multiply anyway, and the compiler's own carry chains carry
// their own wait states; there is no inline asm in this file.  Addition and subtraction are the generic 64-bit forms below.
#pragma once

#include "fr.hpp"  // PG_HD, adc64 / sbb64 / mac64

namespace pg {

struct Fq {
    uint64_t l[6];
};

#define PG_P0 0xb9feffffffffaaabull
#define PG_P1 0x1eabfffeb153ffffull
#define PG_P2 0x6730d2a0f6b0f624ull
#define PG_P3 0x64774b84f38512bfull
#define PG_P4 0x4b1ba7b6434bacd7ull
#define PG_P5 0x1a0111ea397fe69aull
// -p^{-1} mod 2^64 and mod 2^32
#define PG_PINV 0x89f3fffcfffcfffdull
#define PG_PINV32 0xfffcfffdu

PG_HD Fq fq_zero() { return Fq{{0, 0, 0, 0, 0, 0}}; }
// mont(1) = R mod p
PG_HD Fq fq_one() {
    return Fq{{0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull, 0x77ce585370525745ull, 0x5c071a97a256ec6dull,
               0x15f65ec3fa80e493ull}};
}
// R^2 mod p
PG_HD Fq fq_r2() {
    return Fq{{0xf4df1f341c341746ull, 0x0a76e6a609d104f1ull, 0x8de5476c4c95b6d5ull, 0x67eb88a9939d83c0ull, 0x9a793e85b519952dull,
               0x11988fe592cae3aaull}};
}

PG_HD bool fq_is_zero(const Fq &a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3] | a.l[4] | a.l[5]) == 0; }
PG_HD bool fq_eq(const Fq &a, const Fq &b) {
    return ((a.l[0] ^ b.l[0]) | (a.l[1] ^ b.l[1]) | (a.l[2] ^ b.l[2]) | (a.l[3] ^ b.l[3]) | (a.l[4] ^ b.l[4]) | (a.l[5] ^ b.l[5])) == 0;
}
// limbs < p (host validation of caller input)
PG_HD bool fq_is_reduced(const Fq &a) {
    const uint64_t P[6] = {PG_P0, PG_P1, PG_P2, PG_P3, PG_P4, PG_P5};
    for (int i = 5; i >= 0; i--) {
        if (a.l[i] < P[i]) return true;
        if (a.l[i] > P[i]) return false;
    }
    return false;
}

// r (with a virtual 7th limb `top`, value < 2p) -> r mod p
PG_HD Fq fq_final_sub(const uint64_t r[6], uint64_t top) {
    const uint64_t P[6] = {PG_P0, PG_P1, PG_P2, PG_P3, PG_P4, PG_P5};
    uint64_t bw = 0, d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = sbb64(r[i], P[i], bw);
    const bool keep = top < bw;  // borrowed past the top: r < p
    Fq o;
#pragma unroll
    for (int i = 0; i < 6; i++) o.l[i] = keep ? r[i] : d[i];
    return o;
}

PG_HD Fq fq_add(const Fq &a, const Fq &b) {
    uint64_t c = 0, r[6];
#pragma unroll
    for (int i = 0; i < 6; i++) r[i] = adc64(a.l[i], b.l[i], c);
    return fq_final_sub(r, c);
}

PG_HD Fq fq_sub(const Fq &a, const Fq &b) {
    const uint64_t P[6] = {PG_P0, PG_P1, PG_P2, PG_P3, PG_P4, PG_P5};
    uint64_t bw = 0, d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = sbb64(a.l[i], b.l[i], bw);
    const uint64_t m = 0 - bw;
    uint64_t c = 0;
    Fq o;
#pragma unroll
    for (int i = 0; i < 6; i++) o.l[i] = adc64(d[i], P[i] & m, c);
    return o;
}

PG_HD Fq fq_neg(const Fq &a) {
    const uint64_t P[6] = {PG_P0, PG_P1, PG_P2, PG_P3, PG_P4, PG_P5};
    uint64_t bw = 0;
    const uint64_t nz = fq_is_zero(a) ? 0 : ~0ull;
    Fq o;
#pragma unroll
    for (int i = 0; i < 6; i++) o.l[i] = sbb64(P[i], a.l[i], bw) & nz;
    return o;
}

PG_HD Fq fq_dbl(const Fq &a) { return fq_add(a, a); }

// 12-limb product -> Montgomery reduction (6 rounds) -> final conditional subtraction
PG_HD Fq fq_mont_reduce(uint64_t t[12]) {
    const uint64_t P[6] = {PG_P0, PG_P1, PG_P2, PG_P3, PG_P4, PG_P5};
    uint64_t carry2 = 0;
    for (int i = 0; i < 6; i++) {
        uint64_t k = t[i] * PG_PINV, carry = 0;
        (void)mac64(t[i], k, P[0], carry);
        for (int j = 1; j < 6; j++) t[i + j] = mac64(t[i + j], k, P[j], carry);
        t[i + 6] = adc64(t[i + 6], carry2, carry);
        carry2 = carry;
    }
    return fq_final_sub(t + 6, carry2);
}

// generic 6 x 64-bit schoolbook product + reduction (host code; also the reference the device form is tested against)
PG_HD Fq fq_mul64(const Fq &a, const Fq &b) {
    uint64_t t[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 6; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < 6; j++) t[i + j] = mac64(t[i + j], a.l[i], b.l[j], carry);
        t[i + 6] = carry;
    }
    return fq_mont_reduce(t);
}

#if defined(__HIP_DEVICE_COMPILE__)
// gfx950 form: 12 x 32-bit words, CIOS (coarsely integrated operand scanning): for each word a_i of x, t += a_i y, then the
// Montgomery digit m = t_0 (-p^-1) mod 2^32 and t = (t + m p) / 2^32.  Every step is one v_mad_u64_u32 (32 x 32 + 64 -> 64,
// which cannot overflow: (2^32 - 1)^2 + 2 (2^32 - 1) < 2^64); 288 per product.  The loop over the twelve words of x stays
// ROLLED (the word is shifted out of x, so nothing is indexed at run time): fully unrolled, a product is ~1200 instructions
// and a point addition inlines 8 to 14 of them, which made the library's compile time grow by 20 minutes for no gain in issue
// rate.  t stays below 2^413 + 2^413 before each division, 13 words; the value before the final subtraction is < 2p.
__device__ __forceinline__ Fq fq_mul(const Fq &x, const Fq &y) {
    const uint32_t P[12] = {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                            0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};
    uint32_t b[12], t[12];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        b[2 * i] = (uint32_t)y.l[i]; b[2 * i + 1] = (uint32_t)(y.l[i] >> 32);
    }
#pragma unroll
    for (int j = 0; j < 12; j++) t[j] = 0;
    uint32_t t12 = 0;
    uint64_t x0 = x.l[0], x1 = x.l[1], x2 = x.l[2], x3 = x.l[3], x4 = x.l[4], x5 = x.l[5];
#pragma unroll 1
    for (int i = 0; i < 12; i++) {
        const uint32_t ai = (uint32_t)x0;
        x0 = (x0 >> 32) | (x1 << 32); x1 = (x1 >> 32) | (x2 << 32); x2 = (x2 >> 32) | (x3 << 32);
        x3 = (x3 >> 32) | (x4 << 32); x4 = (x4 >> 32) | (x5 << 32); x5 >>= 32;
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            const uint64_t s = (uint64_t)ai * b[j] + ((uint64_t)t[j] + c);
            t[j] = (uint32_t)s;
            c = s >> 32;
        }
        const uint64_t s12 = (uint64_t)t12 + c;  // (< 2^33)
        const uint32_t m = t[0] * PG_PINV32;
        c = ((uint64_t)m * P[0] + t[0]) >> 32;  // (the low word becomes 0)
#pragma unroll
        for (int j = 1; j < 12; j++) {
            const uint64_t s = (uint64_t)m * P[j] + ((uint64_t)t[j] + c);
            t[j - 1] = (uint32_t)s;
            c = s >> 32;
        }
        const uint64_t top = s12 + c;
        t[11] = (uint32_t)top;
        t12 = (uint32_t)(top >> 32);
    }
    uint64_t w[6];
#pragma unroll
    for (int i = 0; i < 6; i++) w[i] = ((uint64_t)t[2 * i + 1] << 32) | t[2 * i];
    return fq_final_sub(w, t12);
}
#else
PG_HD Fq fq_mul(const Fq &a, const Fq &b) { return fq_mul64(a, b); }
#endif

PG_HD Fq fq_square(const Fq &a) { return fq_mul(a, a); }

// canonical integer (raw limbs, < p) -> Montgomery form, and back
PG_HD Fq fq_to_mont(const Fq &raw) { return fq_mul(raw, fq_r2()); }
PG_HD Fq fq_from_mont(const Fq &a) {
    uint64_t t[12] = {a.l[0], a.l[1], a.l[2], a.l[3], a.l[4], a.l[5], 0, 0, 0, 0, 0, 0};
    return fq_mont_reduce(t);
}

// a^(p-2) (0 for 0): square-and-multiply over the fixed exponent.  Only a few inversions run per call -- batches go
// through Montgomery's trick (g1.hpp) -- so the simple power is enough.
PG_HD Fq fq_invert(const Fq &a) {
    const uint64_t E[6] = {PG_P0 - 2, PG_P1, PG_P2, PG_P3, PG_P4, PG_P5};  // p - 2 (p0 >= 2: no borrow)
    Fq res = fq_one();
    bool started = false;
#pragma unroll 1
    for (int e = 5; e >= 0; e--) {
#pragma unroll 1
        for (int i = 63; i >= 0; i--) {
            if (started) res = fq_square(res);
            if ((E[e] >> i) & 1) {
                res = started ? fq_mul(res, a) : a;
                started = true;
            }
        }
    }
    return res;
}

}  // namespace pg
