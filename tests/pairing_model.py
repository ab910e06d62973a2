"""Python-integer model of the BLS12-381 pairing: the yardstick of csrc/fq2.hpp, fq12.hpp, g2.hpp and pairing.hpp.

  Fq2  = Fq[u] / (u^2 + 1): pairs (c0, c1) of integers.
  Fq12 = Fq2[w] / (w^6 - XI), XI = 1 + u: lists of six Fq2 coefficients over w^0 .. w^5 (the direct sextic form; the tower
         Fq6 = Fq2[v] / (v^3 - XI), Fq12 = Fq6[w] / (w^2 - v) is the same field with v = w^2: (c0, c2, c4) + (c1, c3, c5) w).
  G2   = the order-r subgroup of the twist y^2 = x^3 + 4 XI over Fq2; points are (x, y) pairs of Fq2, None the identity.
         A twist point (x', y') stands for (x' / w^2, y' / w^3) on y^2 = x^3 + 4 over Fq12.

The Miller loop is the ate loop over |x| = 0xd201000000010000 with affine line functions, each scaled by w^3 (an element of
the proper subfield Fq4, which the final exponentiation kills): the line through T with slope lam, at P = (xP, yP) in G1, is
    (lam xT - yT)  +  (-lam xP) w^2  +  yP w^3,
so a prepared G2 point is the list of 68 pairs (lam xT - yT, -lam): 63 doubling steps and 5 addition steps.  x is negative: the
loop's value is conjugated at the end.  final_exponentiation_plain is the plain power (p^12 - 1) / r; final_exponentiation_chain
is what the device computes, the CUBE of it (HARD_C = 3)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_model as G  # noqa: E402

P = G.P
R = G.R_FR
X_ABS = 0xD201000000010000  # |x|; x itself is negative
XI = (1, 1)
N_LINES = 68
HARD_C = 3  # the device's final exponentiation computes e(P, Q)^3

# the generator of G2 (zcash / dusk-bls12_381's G2Affine::generator) [DEP-RECALL]; pinned by on_twist and r G2 = O
G2X = (0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
       0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E)
G2Y = (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
       0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE)
G2 = (G2X, G2Y)
B2 = (4, 4)  # 4 XI


# ---- Fq2 ------------------------------------------------------------------------------------------------------------------
def f2_add(a, b):
    return (a[0] + b[0]) % P, (a[1] + b[1]) % P


def f2_sub(a, b):
    return (a[0] - b[0]) % P, (a[1] - b[1]) % P


def f2_neg(a):
    return (-a[0]) % P, (-a[1]) % P


def f2_conj(a):
    return a[0], (-a[1]) % P


def f2_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P


def f2_sqr(a):
    return f2_mul(a, a)


def f2_scale(a, k):
    return a[0] * k % P, a[1] * k % P


def f2_mul_xi(a):
    """a (1 + u)"""
    return (a[0] - a[1]) % P, (a[0] + a[1]) % P


def f2_inv(a):
    """0 for 0, like the library"""
    n = (a[0] * a[0] + a[1] * a[1]) % P
    if n == 0:
        return 0, 0
    ni = pow(n, -1, P)
    return a[0] * ni % P, (-a[1]) * ni % P


def f2_pow(a, e):
    out = (1, 0)
    for bit in bin(e)[2:]:
        out = f2_sqr(out)
        if bit == "1":
            out = f2_mul(out, a)
    return out


def f2_sqrt(a):
    """a square root of a or None (p = 3 mod 4: Adj and Rodriguez-Henriquez, algorithm 9)"""
    if a == (0, 0):
        return 0, 0
    a1 = f2_pow(a, (P - 3) // 4)
    alpha = f2_mul(f2_sqr(a1), a)
    x0 = f2_mul(a1, a)
    if alpha == (P - 1, 0):
        cand = f2_mul((0, 1), x0)
    else:
        cand = f2_mul(f2_pow(f2_add((1, 0), alpha), (P - 1) // 2), x0)
    return cand if f2_sqr(cand) == a else None


# the Frobenius constants: w^(p^n) = GAMMA_n[1] w, so (c w^k)^(p^n) = c^(p^n) GAMMA_n[k] w^k with GAMMA_n[k] = XI^(k (p^n - 1) / 6)
GAMMA1 = [f2_pow(XI, k * (P - 1) // 6) for k in range(6)]
GAMMA2 = [f2_pow(XI, k * (P * P - 1) // 6) for k in range(6)]  # in Fq: the c1 halves are 0
GAMMA3 = [f2_pow(XI, k * (P ** 3 - 1) // 6) for k in range(6)]

# ---- Fq12 -----------------------------------------------------------------------------------------------------------------
F12_ONE = [(1, 0)] + [(0, 0)] * 5
F12_ZERO = [(0, 0)] * 6


def f12_add(a, b):
    return [f2_add(x, y) for x, y in zip(a, b)]


def f12_sub(a, b):
    return [f2_sub(x, y) for x, y in zip(a, b)]


def f12_neg(a):
    return [f2_neg(x) for x in a]


def f12_mul(a, b):
    out = []
    for k in range(6):
        lo, hi = (0, 0), (0, 0)
        for i in range(6):
            j = k - i
            if j >= 0:
                lo = f2_add(lo, f2_mul(a[i], b[j]))
            else:
                hi = f2_add(hi, f2_mul(a[i], b[j + 6]))
        out.append(f2_add(lo, f2_mul_xi(hi)))
    return out


def f12_sqr(a):
    return f12_mul(a, a)


def f12_conj(a):
    """a^(p^6): w -> -w"""
    return [f2_neg(c) if k & 1 else c for k, c in enumerate(a)]


def f12_frobenius(a, n=1):
    """a^(p^n), n = 1, 2 or 3"""
    g = {1: GAMMA1, 2: GAMMA2, 3: GAMMA3}[n]
    return [f2_mul(f2_conj(c) if n & 1 else c, g[k]) for k, c in enumerate(a)]


def f12_mul_sparse(f, l0, l2, l3):
    """f (l0 + l2 w^2 + l3 w^3), l0 and l2 in Fq2, l3 in Fq"""
    line = [l0, (0, 0), l2, (l3 % P, 0), (0, 0), (0, 0)]
    return f12_mul(f, line)


def _f6_mul(a, b):
    a0, a1, a2 = a
    b0, b1, b2 = b
    return [f2_add(f2_mul(a0, b0), f2_mul_xi(f2_add(f2_mul(a1, b2), f2_mul(a2, b1)))),
            f2_add(f2_add(f2_mul(a0, b1), f2_mul(a1, b0)), f2_mul_xi(f2_mul(a2, b2))),
            f2_add(f2_add(f2_mul(a0, b2), f2_mul(a1, b1)), f2_mul(a2, b0))]


def _f6_mul_v(a):
    return [f2_mul_xi(a[2]), a[0], a[1]]


def _f6_inv(a):
    c0, c1, c2 = a
    t0 = f2_sub(f2_sqr(c0), f2_mul_xi(f2_mul(c1, c2)))
    t1 = f2_sub(f2_mul_xi(f2_sqr(c2)), f2_mul(c0, c1))
    t2 = f2_sub(f2_sqr(c1), f2_mul(c0, c2))
    d = f2_add(f2_mul(c0, t0), f2_mul_xi(f2_add(f2_mul(c2, t1), f2_mul(c1, t2))))
    di = f2_inv(d)
    return [f2_mul(t0, di), f2_mul(t1, di), f2_mul(t2, di)]


def f12_inv(a):
    """through the tower: (A + B w)^-1 = (A - B w) / (A^2 - v B^2); 0 for 0"""
    A, B = [a[0], a[2], a[4]], [a[1], a[3], a[5]]
    d = [f2_sub(x, y) for x, y in zip(_f6_mul(A, A), _f6_mul_v(_f6_mul(B, B)))]
    di = _f6_inv(d)
    ra, rb = _f6_mul(A, di), _f6_mul(B, di)
    return [ra[0], f2_neg(rb[0]), ra[1], f2_neg(rb[1]), ra[2], f2_neg(rb[2])]


def f12_pow(a, e):
    out = list(F12_ONE)
    for bit in bin(e)[2:]:
        out = f12_sqr(out)
        if bit == "1":
            out = f12_mul(out, a)
    return out


# ---- G2 (affine, on the twist) ------------------------------------------------------------------------------------------
def on_twist(q) -> bool:
    if q is None:
        return True
    x, y = q
    return f2_sqr(y) == f2_add(f2_mul(f2_sqr(x), x), B2)


def g2_neg(q):
    return None if q is None else (q[0], f2_neg(q[1]))


def _dbl_slope(t):
    return f2_mul(f2_scale(f2_sqr(t[0]), 3), f2_inv(f2_scale(t[1], 2)))


def _chord(t, lam, x2):
    x3 = f2_sub(f2_sub(f2_sqr(lam), t[0]), x2)
    return x3, f2_sub(f2_mul(lam, f2_sub(t[0], x3)), t[1])


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if f2_add(a[1], b[1]) == (0, 0):
            return None
        lam = _dbl_slope(a)
    else:
        lam = f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))
    return _chord(a, lam, b[0])


def g2_mul(k: int, q):
    if q is None or k == 0:
        return None
    if k < 0:
        return g2_mul(-k, g2_neg(q))
    acc = None
    for bit in bin(k)[2:]:
        acc = g2_add(acc, acc)
        if bit == "1":
            acc = g2_add(acc, q)
    return acc


def g2_compressed(q) -> bytes:
    """the 96-byte zcash / dusk-bls12_381 encoding: x.c1 then x.c0, big-endian; bit 7 compressed, bit 6 identity, bit 5 set
    when y is the lexicographically larger of (y, -y), compared by c1 first and then c0"""
    if q is None:
        return bytes([0xC0]) + bytes(95)
    (x0, x1), y = q
    out = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    out[0] |= 0x80
    ny = f2_neg(y)
    if (y[1], y[0]) > (ny[1], ny[0]):
        out[0] |= 0x20
    return bytes(out)


# ---- the Miller loop ----------------------------------------------------------------------------------------------------
LOOP_BITS = [int(b) for b in bin(X_ABS)[3:]]  # the 63 bits below the top one, most significant first


def g2_prepare(q):
    """the 68 lines of the ate loop over q (not the identity): [(lam xT - yT, -lam)], a doubling line per bit and an addition
    line after it for each set bit"""
    lines, t = [], q
    for bit in LOOP_BITS:
        lam = _dbl_slope(t)
        lines.append((f2_sub(f2_mul(lam, t[0]), t[1]), f2_neg(lam)))
        t = _chord(t, lam, t[0])
        if bit:
            lam = f2_mul(f2_sub(t[1], q[1]), f2_inv(f2_sub(t[0], q[0])))
            lines.append((f2_sub(f2_mul(lam, t[0]), t[1]), f2_neg(lam)))
            t = _chord(t, lam, q[0])
    assert len(lines) == N_LINES
    return lines


def miller_loop(pairs):
    """prod_j f_{|x|, Q_j}(P_j), conjugated: pairs of (P, prepared Q); an identity P contributes 1"""
    pairs = [(p, ln) for p, ln in pairs if p is not None]
    f, idx = list(F12_ONE), 0
    for bit in LOOP_BITS:
        f = f12_sqr(f)
        for _ in range(1 + bit):
            for (xp, yp), ln in pairs:
                f = f12_mul_sparse(f, ln[idx][0], f2_scale(ln[idx][1], xp), yp)
            idx += 1
    return f12_conj(f)


def final_exponentiation_plain(f):
    """f^((p^12 - 1) / r)"""
    return f12_pow(f, (P ** 12 - 1) // R)


def easy_part(f):
    """f^((p^6 - 1)(p^2 + 1))"""
    t = f12_mul(f12_conj(f), f12_inv(f))
    return f12_mul(f12_frobenius(t, 2), t)


def _pow_x(a):
    """a^x for the negative x, a in the cyclotomic subgroup (inverse = conjugate)"""
    return f12_conj(f12_pow(a, X_ABS))


def final_exponentiation_chain(f):
    """f^(3 (p^12 - 1) / r), the way the device computes it: the easy part, then the hard part by
    3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3  (Hayashida, Hayasaka and Teruya, 2020)"""
    m = easy_part(f)
    t = f12_mul(_pow_x(m), f12_conj(m))                    # m^(x - 1)
    t = f12_mul(_pow_x(t), f12_conj(t))                    # ^(x - 1)
    t = f12_mul(_pow_x(t), f12_frobenius(t, 1))            # ^(x + p)
    t = f12_mul(f12_mul(_pow_x(_pow_x(t)), f12_frobenius(t, 2)), f12_conj(t))  # ^(x^2 + p^2 - 1)
    return f12_mul(t, f12_mul(f12_sqr(m), m))


def pairing(p, q):
    """e(P, Q) = (the Miller value)^((p^12 - 1) / r); 1 when either is the identity"""
    if p is None or q is None:
        return list(F12_ONE)
    return final_exponentiation_plain(miller_loop([(p, g2_prepare(q))]))


# ---- limbs ----------------------------------------------------------------------------------------------------------------
def f2_limbs(a) -> list:
    return G.fq_limbs(a[0]) + G.fq_limbs(a[1])


def f2_from_limbs(limbs):
    return G.fq_from_limbs(limbs[:6]), G.fq_from_limbs(limbs[6:12])


def f12_limbs(a) -> list:
    return [w for c in a for w in f2_limbs(c)]


def f12_from_limbs(limbs) -> list:
    return [f2_from_limbs(limbs[12 * k:12 * k + 12]) for k in range(6)]


def g2_limbs(q) -> list:
    """the 24 limbs of a pg_g2_affine: x.c0, x.c1, y.c0, y.c1"""
    return [0] * 24 if q is None else f2_limbs(q[0]) + f2_limbs(q[1])


def g2_from_limbs(limbs):
    if not any(int(w) & G.MASK for w in limbs):
        return None
    return f2_from_limbs(limbs[:12]), f2_from_limbs(limbs[12:])
