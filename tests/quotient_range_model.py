"""TEST INFRASTRUCTURE: the quotient with the range widget's term in plain Python integers mod q -- the statement
pg_quotient_range (csrc/quotient.hpp) is compared with, limb for limb.  The conventions of
tests/quotient_model.py and tests/quotient_blinded_model.py, with one more input q_range (n coefficients) and

  N(x) += q_range(x) [ alpha^3 delta(b - 4a) + alpha^4 delta(c - 4b) + alpha^5 delta(a(omega x) - 4c) ],  delta(f) = f (f-1)(f-2)(f-3).

Unblinded: ONE 4n-point coset transform per input (quotient).  Blinded: the definition through ONE 8n-point transform per input
(quotient_blinded), and schoolbook products with long division by X^n - 1 (exact_quotient).  Without "q_range" among the inputs
the results are those of the models this one extends.  Also: model circuits of arithmetic rows and range items (tests/
range_gate_model.py) as the quotient's inputs, built without the library."""
from ntt_model import DEFAULT_G, coset_fft, coset_ifft, horner, ifft
from perm_product_model import K, Q, grand_product, omega_of, sigma_evaluations
import quotient_blinded_model as BM
import quotient_model as QM
import range_gate_model as RG

TOP = BM.TOP


def delta(f: int) -> int:
    return f * (f - 1) * (f - 2) * (f - 3) % Q


def range_term(v: dict, aw: int, alpha: int) -> int:
    """the term at one point from the values there; aw = a(omega x)"""
    s = pow(alpha, 3, Q) * delta(v["b"] - 4 * v["a"]) + pow(alpha, 4, Q) * delta(v["c"] - 4 * v["b"]) + pow(alpha, 5, Q) * delta(aw - 4 * v["c"])
    return v.get("q_range", 0) * s % Q


def numerator(v: dict, zw: int, aw: int, x: int, n: int, alpha: int, beta: int, gamma: int, k=K) -> int:
    return (QM.numerator(v, zw, x, n, alpha, beta, gamma, k) + range_term(v, aw, alpha)) % Q


def quotient(polys: dict, alpha: int, beta: int, gamma: int, k=K, g: int = DEFAULT_G) -> list:
    """polys: those of quotient_model.quotient and optionally q_range, n coefficients each -> t: 4n ints"""
    n = len(polys["z"])
    m = n.bit_length() - 1
    assert n == 1 << m
    zeta = omega_of(m + 2)
    ev = {name: coset_fft(list(c) + [0] * (3 * n), g, zeta) for name, c in polys.items()}
    out, x = [], g % Q
    for i in range(4 * n):
        v = {name: e[i] for name, e in ev.items()}
        j = (i + 4) % (4 * n)  # omega x = zeta^4 x
        out.append(numerator(v, ev["z"][j], ev["a"][j], x, n, alpha, beta, gamma, k) * pow(pow(x, n, Q) - 1, -1, Q) % Q)
        x = x * zeta % Q
    return coset_ifft(out, g, zeta)


# ---- schoolbook ----------------------------------------------------------------------------------------------------------------
def shifted(c, omega: int) -> list:
    """c(omega X)"""
    out, x = [], 1
    for v in c:
        out.append(v * x % Q)
        x = x * omega % Q
    return out


def delta_poly(hi, lo) -> list:
    f = BM.p_add(hi, BM.p_scale(lo, Q - 4))
    out = f
    for c in (1, 2, 3):
        out = BM.p_mul(out, BM.p_add(f, [Q - c]))
    return out


def range_poly(polys: dict, n: int, alpha: int) -> list:
    if "q_range" not in polys:
        return [0]
    a, b, c = polys["a"], polys["b"], polys["c"]
    aw = shifted(a, omega_of(n.bit_length() - 1))
    s = BM.p_scale(delta_poly(b, a), pow(alpha, 3, Q))
    s = BM.p_add(s, BM.p_scale(delta_poly(c, b), pow(alpha, 4, Q)))
    s = BM.p_add(s, BM.p_scale(delta_poly(aw, c), pow(alpha, 5, Q)))
    return BM.p_mul(polys["q_range"], s)


def numerator_poly(polys: dict, n: int, alpha: int, beta: int, gamma: int, k=K) -> list:
    return BM.p_add(BM.numerator_poly(polys, n, alpha, beta, gamma, k), range_poly(polys, n, alpha))


def exact_quotient(polys: dict, alpha: int, beta: int, gamma: int, k=K):
    """-> (t as 4n + 8 coefficients, the division's remainder, deg t); wires of n or n + 2 coefficients, z of n or n + 3"""
    n = len(polys["s1"])
    t, rem = BM.divide_by_vanishing(numerator_poly(polys, n, alpha, beta, gamma, k), n)
    deg = max((i for i, x in enumerate(t) if x), default=-1)
    assert len(t) <= 4 * n + 8
    return t + [0] * (4 * n + 8 - len(t)), rem, deg


# ---- the blinded definition ----------------------------------------------------------------------------------------------------
def numerator_coefficients(polys: dict, alpha: int, beta: int, gamma: int, k=K, g: int = DEFAULT_G) -> list:
    """N's 8n coefficients (deg N <= 5n + 6 < 8n) from its values on a coset of 8n points"""
    n = len(polys["s1"])
    m = n.bit_length() - 1
    assert n == 1 << m and n >= 8
    theta = omega_of(m + 3)
    ev = {name: coset_fft(list(c) + [0] * (8 * n - len(c)), g, theta) for name, c in polys.items()}
    vals, x = [], g % Q
    for i in range(8 * n):
        v = {name: e[i] for name, e in ev.items()}
        j = (i + 8) % (8 * n)  # omega x = theta^8 x
        vals.append(numerator(v, ev["z"][j], ev["a"][j], x, n, alpha, beta, gamma, k))
        x = x * theta % Q
    return coset_ifft(vals, g, theta)


def quotient_blinded(polys: dict, alpha: int, beta: int, gamma: int, k=K, g: int = DEFAULT_G) -> list:
    """polys: those of quotient_blinded_model.quotient_blinded and optionally q_range (n coefficients) -> 4n + 8 ints"""
    n = len(polys["s1"])
    m = n.bit_length() - 1
    assert all(len(polys[w]) == n + 2 for w in BM.WIRES) and len(polys["z"]) == n + 3
    N = numerator_coefficients(polys, alpha, beta, gamma, k, g)
    assert not any(N[5 * n + TOP:])
    T = N[5 * n:5 * n + TOP]
    g4n = pow(g, 4 * n, Q)
    folded = [(N[i] + g4n * N[4 * n + i]) % Q for i in range(4 * n)]
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
    rw = r * omega % Q
    return horner(t, r) * (pow(r, n, Q) - 1) % Q, numerator(v, horner(polys["z"], rw), horner(polys["a"], rw), r, n, alpha, beta, gamma, k)


# ---- model circuits ------------------------------------------------------------------------------------------------------------
class ModelCircuit:
    """rows (a, b, c; q_m, q_l, q_r, q_o, q_c; q_range) over Variables with integer values; the fourth wire is zero_var on every
    row (q_4 = 0) and q_arith = 1.  Variable 0 is zero_var, pinned by row 0 as the composer pins it."""

    def __init__(self):
        self.values = [0]
        self.rows = []
        self.gate(0, 0, 0, q_l=1)

    def add_input(self, v):
        self.values.append(v % Q)
        return len(self.values) - 1

    def gate(self, a, b, c, q_m=0, q_l=0, q_r=0, q_o=0, q_c=0, q_range=0):
        self.rows.append(((a, b, c), tuple(x % Q for x in (q_m, q_l, q_r, q_o, q_c)), q_range))

    def mul(self, a, b):
        c = self.add_input(self.values[a] * self.values[b])
        self.gate(a, b, c, q_m=1, q_o=-1)
        return c

    def range_gate(self, witness, num_bits):
        rows, qr, new = RG.item(witness, self.values[witness], num_bits, len(self.values), 0)
        self.values += new
        for r, q in zip(rows, qr):
            self.gate(*r, q_range=q)

    def sigma(self, padded_n):
        """sigma[w][i] = w' * padded_n + i': the next position of the row's Variable (positions in wire-major order); rows of the
        padding and the fourth wire hold zero_var like every unused wire, joined to its cycle"""
        where = {}
        wires = [[r[0][j] for r in self.rows] + [0] * (padded_n - len(self.rows)) for j in range(3)] + [[0] * padded_n]
        for w in range(4):
            for i in range(padded_n):
                where.setdefault(wires[w][i], []).append(w * padded_n + i)
        sigma = [[0] * padded_n for _ in range(4)]
        for pos in where.values():
            for p, nxt in zip(pos, pos[1:] + pos[:1]):
                sigma[p // padded_n][p % padded_n] = nxt
        return sigma

    def polys(self, padded_n, beta, gamma, values=None):
        """the quotient's inputs as coefficient lists over the padded domain; values: a replacement for the assignments"""
        import numpy as np
        vals = self.values if values is None else values
        n = len(self.rows)
        assert n <= padded_n
        pad = lambda xs: list(xs) + [0] * (padded_n - len(xs))
        m = padded_n.bit_length() - 1
        wires = [pad([vals[r[0][j]] for r in self.rows]) for j in range(3)] + [[0] * padded_n]
        sigma = np.array(self.sigma(padded_n), dtype=np.uint64)
        z, wrap = grand_product(wires, sigma, padded_n, beta, gamma, omega_of(m))
        out = {name: ifft(w) for name, w in zip("abcd", wires)}
        out["z"] = ifft(z)
        for j, s in enumerate(sigma_evaluations(sigma, padded_n, omega_of(m))):
            out["s%d" % (j + 1)] = ifft(s)
        for i, name in enumerate(("q_m", "q_l", "q_r", "q_o", "q_c")):
            out[name] = ifft(pad([r[1][i] for r in self.rows]))
        out["q_4"] = [0] * padded_n
        out["q_arith"] = ifft(pad([1] * n))
        out["q_range"] = ifft(pad([r[2] for r in self.rows]))
        return out, wrap


def range_circuit(padded_n: int, exact: bool = False):
    """a model circuit of a few arithmetic rows and range items of 8, 16 and 6 bits (and, from 32 rows on, 62) that pads to
    padded_n; exact: filled with 2-bit items and arithmetic rows to exactly padded_n rows.  -> (circuit, an accumulator Variable)"""
    c = ModelCircuit()
    x, y = c.add_input(13), c.add_input(15)
    w8 = c.mul(x, y)                       # 195 < 2^8
    first_acc = len(c.values)
    c.range_gate(w8, 8)                    # 3 rows
    if padded_n >= 16:
        c.range_gate(c.add_input(0xBEEF), 16)  # 4 rows
        c.range_gate(c.add_input(63), 6)       # 2 rows
    if padded_n >= 32:
        c.range_gate(c.add_input(2**62 - 12345), 62)  # 12 rows
    assert len(c.rows) <= padded_n and (padded_n == 8 or 2 * len(c.rows) > padded_n), (len(c.rows), padded_n)
    if exact:
        while len(c.rows) + 2 <= padded_n:
            c.range_gate(c.add_input(len(c.rows) % 4), 2)
        while len(c.rows) < padded_n:
            c.mul(x, y)
    return c, first_acc
