// fq2.hpp -- Fq2 = Fq[u] / (u^2 + 1) over fq.hpp, the coefficient field of the pairing's Fq12 (fq12.hpp) and of G2 (g2.hpp).
// Two Fq elements c0 + c1 u, each Montgomery form and fully reduced, so that equal elements have identical limbs.  One
// source for host and gfx950 device code; every product is fq_mul (rolled on the device), so a function
// here stays small when it is inlined.
#pragma once

#include "fq.hpp"

namespace pg {

struct Fq2 {
    Fq c0, c1;
};

PG_HD Fq2 fq2_zero() { return Fq2{fq_zero(), fq_zero()}; }
PG_HD Fq2 fq2_one() { return Fq2{fq_one(), fq_zero()}; }
PG_HD bool fq2_is_zero(const Fq2 &a) { return fq_is_zero(a.c0) && fq_is_zero(a.c1); }
PG_HD bool fq2_eq(const Fq2 &a, const Fq2 &b) { return fq_eq(a.c0, b.c0) && fq_eq(a.c1, b.c1); }
PG_HD Fq2 fq2_add(const Fq2 &a, const Fq2 &b) { return Fq2{fq_add(a.c0, b.c0), fq_add(a.c1, b.c1)}; }
PG_HD Fq2 fq2_sub(const Fq2 &a, const Fq2 &b) { return Fq2{fq_sub(a.c0, b.c0), fq_sub(a.c1, b.c1)}; }
PG_HD Fq2 fq2_neg(const Fq2 &a) { return Fq2{fq_neg(a.c0), fq_neg(a.c1)}; }
PG_HD Fq2 fq2_dbl(const Fq2 &a) { return Fq2{fq_dbl(a.c0), fq_dbl(a.c1)}; }
// a^p
PG_HD Fq2 fq2_conj(const Fq2 &a) { return Fq2{a.c0, fq_neg(a.c1)}; }
// a (1 + u): the non-residue XI of the sextic extension
PG_HD Fq2 fq2_mul_xi(const Fq2 &a) { return Fq2{fq_sub(a.c0, a.c1), fq_add(a.c0, a.c1)}; }
// a k, k in Fq
PG_HD Fq2 fq2_mul_fq(const Fq2 &a, const Fq &k) { return Fq2{fq_mul(a.c0, k), fq_mul(a.c1, k)}; }

// Karatsuba: three Fq products
PG_HD Fq2 fq2_mul(const Fq2 &a, const Fq2 &b) {
    const Fq v0 = fq_mul(a.c0, b.c0), v1 = fq_mul(a.c1, b.c1);
    const Fq m = fq_mul(fq_add(a.c0, a.c1), fq_add(b.c0, b.c1));
    return Fq2{fq_sub(v0, v1), fq_sub(fq_sub(m, v0), v1)};
}

// (c0 + c1)(c0 - c1) + 2 c0 c1 u: two Fq products
PG_HD Fq2 fq2_square(const Fq2 &a) {
    const Fq t = fq_mul(a.c0, a.c1);
    return Fq2{fq_mul(fq_add(a.c0, a.c1), fq_sub(a.c0, a.c1)), fq_dbl(t)};
}

// conj(a) / (c0^2 + c1^2); 0 for 0
PG_HD Fq2 fq2_inverse(const Fq2 &a) {
    const Fq n = fq_invert(fq_add(fq_square(a.c0), fq_square(a.c1)));
    return Fq2{fq_mul(a.c0, n), fq_neg(fq_mul(a.c1, n))};
}

}  // namespace pg
