"""TEST INFRASTRUCTURE: the quotient of BLINDED wire and permutation polynomials in plain Python integers mod q -- the statement
pg_quotient_blinded (csrc/quotient.hpp) is compared with, limb for limb.  The conventions of
tests/quotient_model.py; wire j has n + 2 coefficients, w_j = w_j0 + (b1 X + b0)(X^n - 1), and z has n + 3,
z = z0 + (b2 X^2 + b1 X + b0)(X^n - 1); every other input has n.  N is then a polynomial of degree <= 5n + 6.

Two independent forms:
  * exact_quotient: N's coefficients by schoolbook polynomial products and long division by X^n - 1 -> (t, remainder).  Quadratic,
    for the CPU tests' sizes.
  * quotient_blinded: the DEFINITION for arbitrary (unsatisfied) inputs.  T_i := coefficient 5n + i of N (i < 7); t~ := the
    polynomial of degree < 4n with t~(x) = N(x) / (x^n - 1) on the coset g<zeta> of 4n points; out[4n + i] = T_i, out[4n + 7] = 0,
    out[k] = t~[k] - g^(4n) T_k for k < 7 and out[k] = t~[k] otherwise.  N's coefficients come from its values on a coset of 8n
    points (ONE 8n-point transform per input: no split into chunks of n points, no truncated products), and t~ from N folded
    modulo X^(4n) - g^(4n).  For a satisfied circuit it equals exact_quotient's t."""
from ntt_model import DEFAULT_G, coset_fft, coset_ifft, horner
from perm_product_model import K, Q, omega_of
import quotient_model as QM

WIRES = ("a", "b", "c", "d")
TOP = 7  # coefficients of t from 4n up


def blind(c, n: int, blinders) -> list:
    """c: n coefficients; blinders highest power first ((b1, b0) for a wire, (b2, b1, b0) for z) -> c + (sum_k b_k X^k)(X^n - 1)
    as n + len(blinders) coefficients"""
    assert len(c) == n
    low = list(reversed(blinders))  # b0, b1, ...
    out = list(c) + low
    for i, b in enumerate(low):
        out[i] = (out[i] - b) % Q
    return [x % Q for x in out]


def blind_all(polys: dict, blinders) -> dict:
    """polys of n coefficients each and the 11 blinders in the prover's order a1 a0 b1 b0 c1 c0 d1 d0 z2 z1 z0 -> a copy whose
    wires and z are blinded"""
    n = len(polys["z"])
    out = dict(polys)
    for j, name in enumerate(WIRES):
        out[name] = blind(polys[name], n, blinders[2 * j:2 * j + 2])
    out["z"] = blind(polys["z"], n, blinders[8:11])
    return out


# ---- schoolbook --------------------------------------------------------------------------------------------------------------
def p_mul(a, b) -> list:
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return [v % Q for v in out]


def p_add(a, b) -> list:
    if len(a) < len(b):
        a, b = b, a
    return [(x + (b[i] if i < len(b) else 0)) % Q for i, x in enumerate(a)]


def p_scale(a, s: int) -> list:
    return [x * s % Q for x in a]


def numerator_poly(polys: dict, n: int, alpha: int, beta: int, gamma: int, k=K) -> list:
    """N as a polynomial: its coefficients, by schoolbook products"""
    m = n.bit_length() - 1
    omega = omega_of(m)
    w = [polys[name] for name in WIRES]
    gate = p_mul(p_mul(polys["q_m"], w[0]), w[1])
    for q, x in (("q_l", w[0]), ("q_r", w[1]), ("q_o", w[2]), ("q_4", w[3])):
        gate = p_add(gate, p_mul(polys[q], x))
    gate = p_add(gate, polys["q_c"])
    out = p_add(p_mul(polys["q_arith"], gate), polys.get("pi", [0]))
    z = polys["z"]
    zw, x = [], 1
    for c in z:  # z(omega X)
        zw.append(c * x % Q)
        x = x * omega % Q
    num, den = z, zw
    for j in range(4):
        num = p_mul(num, p_add(w[j], [gamma, beta * k[j] % Q]))
        den = p_mul(den, p_add(p_add(w[j], p_scale(polys["s%d" % (j + 1)], beta)), [gamma]))
    out = p_add(out, p_scale(p_add(num, p_scale(den, Q - 1)), alpha))
    l1 = [pow(n, -1, Q)] * n  # (X^n - 1) / (n (X - 1)) = n^-1 (1 + X + ... + X^(n-1))
    return p_add(out, p_scale(p_mul(p_add(z, [Q - 1]), l1), alpha * alpha % Q))


def divide_by_vanishing(N, n: int):
    """N = t (X^n - 1) + rem with deg rem < n, by long division from the top -> (t, rem)"""
    N = list(N)
    for i in range(len(N) - 1, n - 1, -1):
        N[i - n] = (N[i - n] + N[i]) % Q  # the quotient's coefficient i - n is N[i]; N -= N[i] X^(i-n) (X^n - 1)
    return [x % Q for x in N[n:]], [x % Q for x in N[:n]]


def exact_quotient(polys: dict, alpha: int, beta: int, gamma: int, k=K):
    """-> (t as 4n + 8 coefficients, the division's remainder, deg t)"""
    n = len(polys["s1"])
    t, rem = divide_by_vanishing(numerator_poly(polys, n, alpha, beta, gamma, k), n)
    deg = max((i for i, x in enumerate(t) if x), default=-1)
    assert len(t) <= 4 * n + 8
    return t + [0] * (4 * n + 8 - len(t)), rem, deg


# ---- the definition ----------------------------------------------------------------------------------------------------------
def numerator_coefficients(polys: dict, alpha: int, beta: int, gamma: int, k=K, g: int = DEFAULT_G) -> list:
    """N's 8n coefficients (deg N <= 5n + 6 < 8n) from its values on the coset g<theta>, theta = omega_of(m + 3)"""
    n = len(polys["s1"])
    m = n.bit_length() - 1
    assert n == 1 << m and n >= 8
    theta = omega_of(m + 3)
    ev = {name: coset_fft(list(c) + [0] * (8 * n - len(c)), g, theta) for name, c in polys.items()}
    vals, x = [], g % Q
    for i in range(8 * n):
        v = {name: e[i] for name, e in ev.items()}
        zw = ev["z"][(i + 8) % (8 * n)]  # omega x = theta^8 x
        vals.append(QM.numerator(v, zw, x, n, alpha, beta, gamma, k))
        x = x * theta % Q
    return coset_ifft(vals, g, theta)


def quotient_blinded(polys: dict, alpha: int, beta: int, gamma: int, k=K, g: int = DEFAULT_G) -> list:
    """polys: a, b, c, d (n + 2 coefficients), z (n + 3), s1..s4, the SELECTORS and optionally pi (n) -> 4n + 8 ints"""
    n = len(polys["s1"])
    m = n.bit_length() - 1
    assert all(len(polys[w]) == n + 2 for w in WIRES) and len(polys["z"]) == n + 3
    N = numerator_coefficients(polys, alpha, beta, gamma, k, g)
    assert not any(N[5 * n + TOP:])
    T = N[5 * n:5 * n + TOP]
    g4n = pow(g, 4 * n, Q)
    folded = [(N[i] + g4n * N[4 * n + i]) % Q for i in range(4 * n)]  # N mod (X^(4n) - g^(4n)): N's values on the 4n coset
    zeta = omega_of(m + 2)
    vals, x, q = coset_fft(folded, g, zeta), g % Q, []
    for v in vals:
        q.append(v * pow(pow(x, n, Q) - 1, -1, Q) % Q)
        x = x * zeta % Q
    out = coset_ifft(q, g, zeta)
    for i in range(TOP):
        out[i] = (out[i] - g4n * T[i]) % Q
    return out + T + [0]


def evaluate_at(polys: dict, t: list, r: int, alpha: int, beta: int, gamma: int, k=K):
    """(t(r) (r^n - 1), N(r)) at a point r, from the coefficients (any lengths)"""
    n = len(polys["s1"])
    omega = omega_of(n.bit_length() - 1)
    v = {name: horner(c, r) for name, c in polys.items()}
    zw = horner(polys["z"], r * omega % Q)
    return horner(t, r) * (pow(r, n, Q) - 1) % Q, QM.numerator(v, zw, r, n, alpha, beta, gamma, k)
