// g2.hpp -- BLS12-381 G2 on the HOST: points of the twist y^2 = x^3 + 4 (1 + u) over Fq2 (fq2.hpp), and the prepared form a
// pairing consumes.  G2 work happens once per key (tau G2, the two prepared points of an opening key), never per proof, so the
// arithmetic is the plain affine chord-and-tangent law with one Fq2 inversion per step; the device never does G2 arithmetic.
//   G2A      the ABI's pg_g2_affine: x.c0, x.c1, y.c0, y.c1, Montgomery form, fully reduced; (0, 0) is the identity (not on
//            the twist).  192 bytes.
//   G2Line   one line of the ate Miller loop over Q, ready to be evaluated at any P = (xP, yP) of G1 as
//            c0 + (c2 xP) w^2 + yP w^3 (the line through T with slope lam, scaled by w^3, which lies in the proper subfield Fq4 and
//            dies in the final exponentiation): c0 = lam xT - yT, c2 = -lam.  g2_prepare writes the loop's 68 lines: a doubling
//            step per bit of |x| = 0xd201000000010000 below the top one, an addition step after each set bit.
#pragma once

#include "fq12.hpp"

namespace pg {

struct G2A {
    Fq2 x, y;
};
struct G2Line {
    Fq2 c0, c2;
};

constexpr uint64_t kAteLoop = 0xd201000000010000ull;  // |x|; x is negative
constexpr int kAteLines = 68;

inline bool g2a_is_identity(const G2A &p) { return fq2_is_zero(p.x) && fq2_is_zero(p.y); }
inline G2A g2a_identity() { return G2A{fq2_zero(), fq2_zero()}; }
inline G2A g2a_neg(const G2A &p) { return G2A{p.x, fq2_neg(p.y)}; }
inline bool g2a_eq(const G2A &a, const G2A &b) { return fq2_eq(a.x, b.x) && fq2_eq(a.y, b.y); }

inline G2A g2_generator() {
    const uint64_t t[4][6] = PG_G2_GENERATOR;
    G2A g;
    Fq *f[4] = {&g.x.c0, &g.x.c1, &g.y.c0, &g.y.c1};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 6; j++) f[i]->l[j] = t[i][j];
    return g;
}

// y^2 = x^3 + 4 (1 + u); the identity counts as on the curve
inline bool g2a_on_curve(const G2A &p) {
    if (g2a_is_identity(p)) return true;
    const Fq four = Fq{PG_FQ_FOUR};
    const Fq2 rhs = fq2_add(fq2_mul(fq2_square(p.x), p.x), Fq2{four, four});
    return fq2_eq(fq2_square(p.y), rhs);
}

// the tangent's slope at t: 3 x^2 / (2 y)
inline Fq2 g2_tangent_slope(const G2A &t) {
    const Fq2 x2 = fq2_square(t.x);
    return fq2_mul(fq2_add(fq2_dbl(x2), x2), fq2_inverse(fq2_dbl(t.y)));
}
// the third point of the line through t with slope lam whose other point has abscissa x2
inline G2A g2_chord(const G2A &t, const Fq2 &lam, const Fq2 &x2) {
    const Fq2 x3 = fq2_sub(fq2_sub(fq2_square(lam), t.x), x2);
    return G2A{x3, fq2_sub(fq2_mul(lam, fq2_sub(t.x, x3)), t.y)};
}

inline G2A g2a_add(const G2A &a, const G2A &b) {
    if (g2a_is_identity(a)) return b;
    if (g2a_is_identity(b)) return a;
    Fq2 lam;
    if (fq2_eq(a.x, b.x)) {
        if (fq2_is_zero(fq2_add(a.y, b.y))) return g2a_identity();
        lam = g2_tangent_slope(a);
    } else {
        lam = fq2_mul(fq2_sub(b.y, a.y), fq2_inverse(fq2_sub(b.x, a.x)));
    }
    return g2_chord(a, lam, b.x);
}

// k p for the canonical (not Montgomery) scalar k, double-and-add from the top bit
inline G2A g2a_mul(const G2A &p, const uint64_t k[4]) {
    G2A acc = g2a_identity();
    for (int i = 255; i >= 0; i--) {
        acc = g2a_add(acc, acc);
        if ((k[i / 64] >> (i % 64)) & 1) acc = g2a_add(acc, p);
    }
    return acc;
}

// the 68 lines of the ate loop over q (on the twist, of order r, not the identity)
inline void g2_prepare(const G2A &q, G2Line out[kAteLines]) {
    G2A t = q;
    int n = 0;
    for (int b = 62; b >= 0; b--) {
        Fq2 lam = g2_tangent_slope(t);
        out[n++] = G2Line{fq2_sub(fq2_mul(lam, t.x), t.y), fq2_neg(lam)};
        t = g2_chord(t, lam, t.x);
        if ((kAteLoop >> b) & 1) {
            lam = fq2_mul(fq2_sub(t.y, q.y), fq2_inverse(fq2_sub(t.x, q.x)));
            out[n++] = G2Line{fq2_sub(fq2_mul(lam, t.x), t.y), fq2_neg(lam)};
            t = g2_chord(t, lam, q.x);
        }
    }
}

}  // namespace pg
