// g1_codec.hpp -- G1 ingestion: the 48-byte zcash / dusk-bls12_381 encoding of a G1 point decoded and
// encoded, and the membership test of the order-r subgroup.  The per-point routines are PG_HD over fq.hpp and g1.hpp, so the
// kernels below, the host entry points of capi_codec.inc and the host build of tests/cpp/codec_host.cpp run the same code.
//
//   decode   bytes -> limbs, flags, x < p, Montgomery form, y = (x^3 + 4)^((p + 1) / 4) by a fixed 2-bit window over the constant
//            exponent (378 squarings, 156 products by x, x^2 or x^3 -- the first of the 157 non-zero windows only assigns -- and 2 for
//            x^2 and x^3 themselves: 536; nothing indexed at run time, no table in memory),
//            y^2 == x^3 + 4, the sign from bit 5 against (p - 1) / 2.
//   member   phi(P) = [lambda] P with phi(x, y) = (beta x, y) and lambda = -u^2, u = -0xd201000000010000.  phi^2 + phi + 1 = 0 on
//            the whole curve, so a P that passes satisfies (u^4 - u^2 + 1) P = r P = O; a P of G1 passes because phi acts on G1
//            as one of the two roots of lambda^2 + lambda + 1 mod r, and beta is the cube root of unity that goes with -u^2
//            (tests/g1_codec_model.py pins the pair on the generator).  [u^2] P is [|u|] [|u|] P: 2 x (63 doublings + 5
//            additions), half the doublings of r P and a thirteenth of its additions.  The additions are g1.hpp's complete
//            ones: points of small order do reach P = +-Q and the identity.
//   encode   the inverse of decode (pg_g1_to_compressed's rule).
//
// Words: a point's 48 bytes are handled as six 64-bit words read as the machine reads them (little-endian hosts and gfx950
// alike); the encoding is big-endian, so limb 5 - i of x is the byte-swapped word i and the flags are the top three bits of the
// low byte of word 0.
#pragma once

#if defined(__HIPCC__)
#include "emit.hpp"  // kThreads
#endif
#include "g1.hpp"

namespace pg {

// the per-point status bytes (PG_G1_* of the C ABI)
constexpr uint8_t kG1Ok = 0, kG1BadEncoding = 1, kG1NotOnCurve = 2, kG1NotInSubgroup = 3, kG1NotReduced = 4;

struct G1Bytes {
    uint64_t w[6];
};

// mont(beta), beta = 0x5f19672f...fffefffe: the cube root of unity with (beta x, y) = [-u^2] (x, y) on G1
PG_HD Fq fq_beta() {
    return Fq{{0x30f1361b798a64e8ull, 0xf3b8ddab7ece5a2aull, 0x16a8ca3ac61577f7ull, 0xc26a2ff874fd029bull, 0x3636b76660701c6eull,
               0x051ba4ab241b6160ull}};
}
// mont(4)
PG_HD Fq fq_curve_b() {
    const Fq two = fq_dbl(fq_one());
    return fq_dbl(two);
}

// a canonical (not Montgomery) value > (p - 1) / 2
PG_HD bool fq_canonical_is_high(const Fq &c) {
    const uint64_t H[6] = {0xdcff7fffffffd555ull, 0x0f55ffff58a9ffffull, 0xb39869507b587b12ull,
                           0xb23ba5c279c2895full, 0x258dd3db21a5d66bull, 0x0d0088f51cbff34dull};
    bool greater = false, decided = false;
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        if (!decided && c.l[i] != H[i]) {
            greater = c.l[i] > H[i];
            decided = true;
        }
    }
    return greater;
}

// a^((p + 1) / 4): a square root of a when a is a square (p = 3 mod 4).  2-bit windows from the top of the constant exponent;
// every lane takes the same branches.
PG_HD Fq fq_sqrt_candidate(const Fq &a) {
    const uint64_t E[6] = {0xee7fbfffffffeaabull, 0x07aaffffac54ffffull, 0xd9cc34a83dac3d89ull,
                           0xd91dd2e13ce144afull, 0x92c6e9ed90d2eb35ull, 0x0680447a8e5ff9a6ull};
    const Fq a2 = fq_square(a), a3 = fq_mul(a2, a);
    Fq res = fq_one();
    bool started = false;
#pragma unroll 1
    for (int e = 5; e >= 0; e--) {
#pragma unroll 1
        for (int i = 62; i >= 0; i -= 2) {
            if (started) res = fq_square(fq_square(res));
            const uint32_t d = (uint32_t)(E[e] >> i) & 3u;
            if (d) {
                const Fq m = d == 1 ? a : d == 2 ? a2 : a3;
                res = started ? fq_mul(res, m) : m;
                started = true;
            }
        }
    }
    return res;
}

PG_HD bool g1a_is_reduced(const G1A &p) { return fq_is_reduced(p.x) && fq_is_reduced(p.y); }

// y^2 == x^3 + 4 (the identity (0, 0) is not on the curve: callers test for it first)
PG_HD bool g1a_on_curve(const G1A &p) {
    const Fq rhs = fq_add(fq_mul(fq_square(p.x), p.x), fq_curve_b());
    return fq_eq(fq_square(p.y), rhs);
}

// |u| P, |u| = 0xd201000000010000 (bits 63, 62, 60, 57, 48, 16)
PG_HD G1X g1x_mul_u(const G1X &p) {
    const uint64_t U = 0xd201000000010000ull;
    G1X acc = p;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        acc = g1x_dbl(acc);
        if ((U >> i) & 1) acc = g1x_add(acc, p);
    }
    return acc;
}

// for a point ON THE CURVE that is not the identity: [u^2] P == -phi(P) = (beta x, -y), compared without an inversion
PG_HD bool g1a_in_subgroup(const G1A &p) {
    G1X q = g1x_from_affine(p);
#pragma unroll 1
    for (int k = 0; k < 2; k++) q = g1x_mul_u(q);
    if (g1x_is_identity(q)) return false;
    const Fq bx = fq_mul(fq_mul(fq_beta(), p.x), q.zz), ny = fq_mul(fq_neg(p.y), q.zzz);
    return fq_eq(q.x, bx) && fq_eq(q.y, ny);
}

// the status of an affine point as a member of G1: limbs below p, on the curve, of order dividing r (the identity is a member)
PG_HD uint8_t g1a_check(const G1A &p) {
    if (!g1a_is_reduced(p)) return kG1NotReduced;
    if (g1a_is_identity(p)) return kG1Ok;
    if (!g1a_on_curve(p)) return kG1NotOnCurve;
    return g1a_in_subgroup(p) ? kG1Ok : kG1NotInSubgroup;
}

// 48 bytes -> a point and its status; anything but kG1Ok leaves the identity in *out
PG_HD uint8_t g1_decode(const G1Bytes &b, bool check_subgroup, G1A *out) {
    *out = g1a_identity();
    const uint32_t flags = (uint32_t)b.w[0] & 0xe0u;
    if (!(flags & 0x80u)) return kG1BadEncoding;  // not the compressed form
    if (flags & 0x40u) {                          // the identity: exactly c0 00 .. 00
        const uint64_t rest = (b.w[0] ^ 0xc0u) | b.w[1] | b.w[2] | b.w[3] | b.w[4] | b.w[5];
        return rest ? kG1BadEncoding : kG1Ok;
    }
    Fq raw;
#pragma unroll
    for (int i = 0; i < 6; i++) raw.l[5 - i] = __builtin_bswap64(i == 0 ? b.w[0] & ~0xe0ull : b.w[i]);
    if (!fq_is_reduced(raw)) return kG1BadEncoding;  // x >= p
    const Fq x = fq_to_mont(raw);
    const Fq rhs = fq_add(fq_mul(fq_square(x), x), fq_curve_b());
    Fq y = fq_sqrt_candidate(rhs);
    if (!fq_eq(fq_square(y), rhs)) return kG1NotOnCurve;
    if (fq_canonical_is_high(fq_from_mont(y)) != ((flags & 0x20u) != 0)) y = fq_neg(y);
    const G1A p{x, y};
    if (check_subgroup && !g1a_in_subgroup(p)) return kG1NotInSubgroup;
    *out = p;
    return kG1Ok;
}

// a point (reduced limbs) -> its 48 bytes
PG_HD G1Bytes g1_encode(const G1A &p) {
    G1Bytes b;
    if (g1a_is_identity(p)) {
        b.w[0] = 0xc0;
#pragma unroll
        for (int i = 1; i < 6; i++) b.w[i] = 0;
        return b;
    }
    const Fq x = fq_from_mont(p.x);
#pragma unroll
    for (int i = 0; i < 6; i++) b.w[i] = __builtin_bswap64(x.l[5 - i]);
    b.w[0] |= fq_canonical_is_high(fq_from_mont(p.y)) ? 0xa0u : 0x80u;
    return b;
}

#if defined(__HIPCC__)
// One lane per point, grid-stride; nothing waits on another lane or workgroup.  first_bad holds n before the launch
// (g1_first_bad_init_kernel) and the smallest index whose status is not kG1Ok after it.

__global__ void g1_first_bad_init_kernel(unsigned long long *first_bad, unsigned long long n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *first_bad = n;
}

__device__ __forceinline__ G1Bytes g1_load_bytes(const uint4 *in, uint64_t i) {
    const uint4 a = in[3 * i], b = in[3 * i + 1], c = in[3 * i + 2];
    return G1Bytes{{(uint64_t)a.y << 32 | a.x, (uint64_t)a.w << 32 | a.z, (uint64_t)b.y << 32 | b.x, (uint64_t)b.w << 32 | b.z,
                    (uint64_t)c.y << 32 | c.x, (uint64_t)c.w << 32 | c.z}};
}

__global__ __launch_bounds__(kThreads) void g1_decompress_kernel(const uint4 *in, uint64_t n, uint32_t check_subgroup, G1A *out,
                                                                 uint8_t *status, unsigned long long *first_bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        G1A p;
        const uint8_t st = g1_decode(g1_load_bytes(in, i), check_subgroup != 0, &p);
        out[i] = p;
        status[i] = st;
        if (st != kG1Ok) atomicMin(first_bad, (unsigned long long)i);
    }
}

__global__ __launch_bounds__(kThreads) void g1_check_kernel(const G1A *points, uint64_t n, uint8_t *status, unsigned long long *first_bad) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const uint8_t st = g1a_check(points[i]);
        status[i] = st;
        if (st != kG1Ok) atomicMin(first_bad, (unsigned long long)i);
    }
}

__global__ __launch_bounds__(kThreads) void g1_compress_kernel(const G1A *points, uint64_t n, uint4 *out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const G1Bytes b = g1_encode(points[i]);
        out[3 * i] = uint4{(uint32_t)b.w[0], (uint32_t)(b.w[0] >> 32), (uint32_t)b.w[1], (uint32_t)(b.w[1] >> 32)};
        out[3 * i + 1] = uint4{(uint32_t)b.w[2], (uint32_t)(b.w[2] >> 32), (uint32_t)b.w[3], (uint32_t)(b.w[3] >> 32)};
        out[3 * i + 2] = uint4{(uint32_t)b.w[4], (uint32_t)(b.w[4] >> 32), (uint32_t)b.w[5], (uint32_t)(b.w[5] >> 32)};
    }
}
#endif

}  // namespace pg
