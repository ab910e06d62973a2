// g1.hpp -- BLS12-381 G1: points on y^2 = x^3 + 4 over Fq (fq.hpp).
//   G1A   the ABI's pg_g1_affine: Montgomery-form, fully reduced coordinates; (0, 0) is the identity (not on the curve, so it
//         cannot collide with a real point).  96 bytes.
//   G1X   the accumulator: XYZZ coordinates (x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2); ZZ = 0 is the identity.  The
//         formulas are the "xyzz" ones of the Explicit-Formulas Database (madd-2008-s, add-2008-s, dbl-2008-s-1,
//         mdbl-2008-s-1); each addition below also handles P + P (it doubles), P + (-P) and the identity on either side.
// Batch normalisation (one inversion per batch, Montgomery's trick) is g1_normalize_kernel in msm.hpp.
#pragma once

#include "fq.hpp"

namespace pg {

struct G1A {
    Fq x, y;
};
struct G1X {
    Fq x, y, zz, zzz;
};

PG_HD bool g1a_is_identity(const G1A &p) { return fq_is_zero(p.x) && fq_is_zero(p.y); }
PG_HD bool g1x_is_identity(const G1X &p) { return fq_is_zero(p.zz); }
PG_HD G1X g1x_identity() { return G1X{fq_zero(), fq_zero(), fq_zero(), fq_zero()}; }
PG_HD G1A g1a_identity() { return G1A{fq_zero(), fq_zero()}; }
PG_HD G1A g1a_neg(const G1A &p) { return G1A{p.x, fq_neg(p.y)}; }  // (fq_neg(0) = 0: the identity stays itself)
PG_HD G1X g1x_from_affine(const G1A &p) {
    if (g1a_is_identity(p)) return g1x_identity();
    return G1X{p.x, p.y, fq_one(), fq_one()};
}

// the generator of dusk-bls12_381 (G1Affine::generator), Montgomery form
PG_HD G1A g1_generator() {
    return G1A{Fq{{0x5cb38790fd530c16ull, 0x7817fc679976fff5ull, 0x154f95c7143ba1c1ull, 0xf0ae6acdf3d0e747ull, 0xedce6ecc21dbf440ull,
                   0x120177419e0bfb75ull}},
               Fq{{0xbaac93d50ce72271ull, 0x8c22631a7918fd8eull, 0xdd595f13570725ceull, 0x51ac582950405194ull, 0x0e1c8c3fad0059c0ull,
                   0x0bbc3efc5008a26aull}}};
}

// 2P (dbl-2008-s-1, a = 0); a point with y = 0 would give ZZ = 0, the identity (E(Fq) has no such point: its order is odd)
PG_HD G1X g1x_dbl(const G1X &p) {
    const Fq u = fq_dbl(p.y), v = fq_square(u), w = fq_mul(u, v), s = fq_mul(p.x, v);
    const Fq x2 = fq_square(p.x), m = fq_add(fq_dbl(x2), x2);
    const Fq x3 = fq_sub(fq_square(m), fq_dbl(s));
    const Fq y3 = fq_sub(fq_mul(m, fq_sub(s, x3)), fq_mul(w, p.y));
    return G1X{x3, y3, fq_mul(v, p.zz), fq_mul(w, p.zzz)};
}

// 2Q for an affine Q that is not the identity (mdbl-2008-s-1)
PG_HD G1X g1x_dbl_affine(const G1A &q) {
    const Fq u = fq_dbl(q.y), v = fq_square(u), w = fq_mul(u, v), s = fq_mul(q.x, v);
    const Fq x2 = fq_square(q.x), m = fq_add(fq_dbl(x2), x2);
    const Fq x3 = fq_sub(fq_square(m), fq_dbl(s));
    const Fq y3 = fq_sub(fq_mul(m, fq_sub(s, x3)), fq_mul(w, q.y));
    return G1X{x3, y3, v, w};
}

// P + Q, Q affine (madd-2008-s): 8 multiplications and 2 squarings in the general case
PG_HD G1X g1x_add_affine(const G1X &p, const G1A &q) {
    if (g1a_is_identity(q)) return p;
    if (g1x_is_identity(p)) return G1X{q.x, q.y, fq_one(), fq_one()};
    const Fq u2 = fq_mul(q.x, p.zz), s2 = fq_mul(q.y, p.zzz);
    const Fq pp_ = fq_sub(u2, p.x), r = fq_sub(s2, p.y);
    if (fq_is_zero(pp_)) {
        if (fq_is_zero(r)) return g1x_dbl_affine(q);  // P = Q
        return g1x_identity();                         // P = -Q
    }
    const Fq pp = fq_square(pp_), ppp = fq_mul(pp_, pp), qq = fq_mul(p.x, pp);
    const Fq x3 = fq_sub(fq_sub(fq_square(r), ppp), fq_dbl(qq));
    const Fq y3 = fq_sub(fq_mul(r, fq_sub(qq, x3)), fq_mul(p.y, ppp));
    return G1X{x3, y3, fq_mul(p.zz, pp), fq_mul(p.zzz, ppp)};
}

// P + Q (add-2008-s): 12 multiplications and 2 squarings in the general case
PG_HD G1X g1x_add(const G1X &p, const G1X &q) {
    if (g1x_is_identity(q)) return p;
    if (g1x_is_identity(p)) return q;
    const Fq u1 = fq_mul(p.x, q.zz), u2 = fq_mul(q.x, p.zz);
    const Fq s1 = fq_mul(p.y, q.zzz), s2 = fq_mul(q.y, p.zzz);
    const Fq pp_ = fq_sub(u2, u1), r = fq_sub(s2, s1);
    if (fq_is_zero(pp_)) {
        if (fq_is_zero(r)) return g1x_dbl(p);
        return g1x_identity();
    }
    const Fq pp = fq_square(pp_), ppp = fq_mul(pp_, pp), qq = fq_mul(u1, pp);
    const Fq x3 = fq_sub(fq_sub(fq_square(r), ppp), fq_dbl(qq));
    const Fq y3 = fq_sub(fq_mul(r, fq_sub(qq, x3)), fq_mul(s1, ppp));
    return G1X{x3, y3, fq_mul(fq_mul(p.zz, q.zz), pp), fq_mul(fq_mul(p.zzz, q.zzz), ppp)};
}

// k P for a small non-negative k (bits < 32), double-and-add from the top bit
PG_HD G1X g1x_mul_small(const G1X &p, uint32_t k) {
    G1X acc = g1x_identity();
#pragma unroll 1
    for (int i = 31; i >= 0; i--) {
        acc = g1x_dbl(acc);
        if ((k >> i) & 1) acc = g1x_add(acc, p);
    }
    return acc;
}

}  // namespace pg
