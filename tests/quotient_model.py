"""TEST INFRASTRUCTURE: PLONK's quotient polynomial in plain Python integers mod q -- the statement pg_quotient (csrc/quotient.hpp)
is compared with, limb for limb.  Conventions [DEP-RECALL] of dusk-plonk 0.8's quotient_poly::compute: n = 2^m, zeta = omega_of(m + 2)
(zeta^4 = omega), g the coset generator, k the wire coset constants; at x on the coset g<zeta> of 4n points
  N(x) = q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c) + PI
       + alpha [ prod_j (w_j + beta k_j x + gamma) z(x) - prod_j (w_j + beta sigma_j + gamma) z(omega x) ]
       + alpha^2 (z(x) - 1) L1(x),        L1(x) = (x^n - 1) / (n (x - 1))
  t = the polynomial of degree < 4n with t(x) = N(x) / (x^n - 1) on those points: t_lo | t_mid | t_hi | t_4th.
Unlike the device, the model evaluates on the whole coset with ONE 4n-point coset transform (tests/ntt_model.py), so a comparison
tests the device's split into four cosets of n points."""
from ntt_model import DEFAULT_G, coset_fft, coset_ifft, horner
from perm_product_model import K, Q, omega_of

SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith")


def numerator(v: dict, zw: int, x: int, n: int, alpha: int, beta: int, gamma: int, k=K) -> int:
    """N at one point x from the values there: v maps a, b, c, d, z, s1..s4 and the SELECTORS (and pi) to ints; zw = z(omega x)"""
    w = [v["a"], v["b"], v["c"], v["d"]]
    gate = (v["q_m"] * w[0] * w[1] + v["q_l"] * w[0] + v["q_r"] * w[1] + v["q_o"] * w[2] + v["q_4"] * w[3] + v["q_c"]) % Q
    num, den = v["z"], zw
    for j in range(4):
        num = num * (w[j] + beta * k[j] * x + gamma) % Q
        den = den * (w[j] + beta * v["s%d" % (j + 1)] + gamma) % Q
    l1 = (pow(x, n, Q) - 1) * pow(n * (x - 1), -1, Q) % Q
    return (v["q_arith"] * gate + v.get("pi", 0) + alpha * (num - den) + alpha * alpha % Q * (v["z"] - 1) * l1) % Q


def quotient(polys: dict, alpha: int, beta: int, gamma: int, k=K, g: int = DEFAULT_G) -> list:
    """polys: a, b, c, d, z, s1..s4, the SELECTORS and optionally pi -> n coefficients each (ints) -> t: 4n ints"""
    n = len(polys["z"])
    m = n.bit_length() - 1
    assert n == 1 << m
    zeta = omega_of(m + 2)
    ev = {name: coset_fft(list(c) + [0] * (3 * n), g, zeta) for name, c in polys.items()}
    out, x, zeta_i = [], g % Q, 1
    for i in range(4 * n):
        v = {name: e[i] for name, e in ev.items()}
        zw = ev["z"][(i + 4) % (4 * n)]  # omega x = zeta^4 x
        out.append(numerator(v, zw, x, n, alpha, beta, gamma, k) * pow(pow(x, n, Q) - 1, -1, Q) % Q)
        x = x * zeta % Q
    return coset_ifft(out, g, zeta)


def evaluate_at(polys: dict, t: list, r: int, alpha: int, beta: int, gamma: int, k=K):
    """(t(r) (r^n - 1), N(r)) at a point r outside H, from the coefficients (equal iff t times the vanishing polynomial is N,
    for all but a negligible share of r)"""
    n = len(polys["z"])
    omega = omega_of(n.bit_length() - 1)
    v = {name: horner(c, r) for name, c in polys.items()}
    zw = horner(polys["z"], r * omega % Q)
    return horner(t, r) * (pow(r, n, Q) - 1) % Q, numerator(v, zw, r, n, alpha, beta, gamma, k)


def identity_from_values(v: dict, zw: int, t_pieces: list, r: int, n: int, alpha: int, beta: int, gamma: int, k=K) -> bool:
    """the same identity from values at r already computed (e.g. by Engine.evaluate): t_pieces = t_lo(r) .. t_4th(r)"""
    rn = pow(r, n, Q)
    t = (t_pieces[0] + rn * t_pieces[1] + rn * rn * t_pieces[2] + pow(rn, 3, Q) * t_pieces[3]) % Q
    return t * (rn - 1) % Q == numerator(v, zw, r, n, alpha, beta, gamma, k)
