"""CPU: the model of the quotient with the range widget's term (tests/quotient_range_model.py).  On model circuits with range
items padded to n = 8, 16 and 32 (one of them filled to exactly n rows), unblinded and with random blinders: the division by
X^n - 1 leaves no remainder, t Z_H = N at a random point, the transform forms equal the schoolbook one, a changed accumulator
breaks both, and a blinded t has 4n <= deg t <= 4n + 6.  On random inputs the definition's T_i are the schoolbook coefficients
5n + i of N, of which the range term feeds the first four.  Without q_range (or with q_range = 0) the results are those of
tests/quotient_model.py and tests/quotient_blinded_model.py."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perm_product_model as M  # noqa: E402
import quotient_blinded_model as BM  # noqa: E402
import quotient_model as QM  # noqa: E402
import quotient_range_model as RM  # noqa: E402

Q = M.Q
ALPHA, BETA, GAMMA = 0x5EED_0051 ** 7 % Q, 0x5EED_0052 ** 9 % Q, 0x5EED_0053 ** 11 % Q
XI = 0x5EED_0054 ** 13 % Q
CASES = [(8, False), (8, True), (16, False), (32, False)]
NAMES = ["a", "b", "c", "d", "z", "s1", "s2", "s3", "s4"] + list(QM.SELECTORS) + ["pi", "q_range"]


def blinders(seed):
    r = random.Random(seed)
    return [r.randrange(Q) for _ in range(11)]


@pytest.mark.parametrize("n,exact", CASES)
def test_satisfied_range_circuit(n, exact):
    circ, acc = RM.range_circuit(n, exact)
    assert not exact or len(circ.rows) == n
    polys, wrap = circ.polys(n, BETA, GAMMA)
    assert wrap == 1 and any(polys["q_range"])
    # unblinded
    t = RM.quotient(polys, ALPHA, BETA, GAMMA)
    te, rem, deg = RM.exact_quotient(polys, ALPHA, BETA, GAMMA)
    assert not any(rem) and te[:4 * n] == t and not any(te[4 * n:])
    lhs, rhs = RM.evaluate_at(polys, t, XI, ALPHA, BETA, GAMMA)
    assert lhs == rhs
    # the range term is needed: without it the same t is not N / Z_H
    lhs, rhs = BM.evaluate_at({k: v for k, v in polys.items() if k != "q_range"}, t, XI, ALPHA, BETA, GAMMA)
    assert lhs != rhs
    # blinded
    bl = BM.blind_all(polys, blinders(n))
    tb, rem, deg = RM.exact_quotient(bl, ALPHA, BETA, GAMMA)
    assert not any(rem) and 4 * n <= deg <= 4 * n + 6 and tb[4 * n + 7] == 0
    assert RM.quotient_blinded(bl, ALPHA, BETA, GAMMA) == tb
    lhs, rhs = RM.evaluate_at(bl, tb, XI, ALPHA, BETA, GAMMA)
    assert lhs == rhs


@pytest.mark.parametrize("n,exact", CASES)
def test_a_changed_accumulator_breaks_the_identity(n, exact):
    circ, acc = RM.range_circuit(n, exact)
    vals = list(circ.values)
    vals[acc] = (vals[acc] + 4) % Q  # 195 >> 6 = 3 -> 7: no quad any more; the copy constraints still hold (one Variable)
    polys, wrap = circ.polys(n, BETA, GAMMA, values=vals)
    assert wrap == 1
    t = RM.quotient(polys, ALPHA, BETA, GAMMA)
    _, rem, _ = RM.exact_quotient(polys, ALPHA, BETA, GAMMA)
    assert any(rem)
    lhs, rhs = RM.evaluate_at(polys, t, XI, ALPHA, BETA, GAMMA)
    assert lhs != rhs
    bl = BM.blind_all(polys, blinders(n + 1))
    tb, rem, _ = RM.exact_quotient(bl, ALPHA, BETA, GAMMA)
    assert any(rem)
    lhs, rhs = RM.evaluate_at(bl, RM.quotient_blinded(bl, ALPHA, BETA, GAMMA), XI, ALPHA, BETA, GAMMA)
    assert lhs != rhs


@pytest.mark.parametrize("n", [8, 16])
def test_random_inputs_top_coefficients_are_the_schoolbook_ones(n):
    r = random.Random(n)
    polys = {name: [r.randrange(Q) for _ in range(n + (2 if name in BM.WIRES else 3 if name == "z" else 0))] for name in NAMES}
    out = RM.quotient_blinded(polys, ALPHA, BETA, GAMMA)
    N = RM.numerator_poly(polys, n, ALPHA, BETA, GAMMA)
    assert len(N) <= 5 * n + 7
    N += [0] * (5 * n + 7 - len(N))
    assert out[4 * n:4 * n + 7] == N[5 * n:5 * n + 7] and out[4 * n + 7] == 0
    # the range term reaches coefficients 5n .. 5n + 3 and no further
    base = BM.numerator_poly(polys, n, ALPHA, BETA, GAMMA)
    rng = RM.range_poly(polys, n, ALPHA)
    assert len(rng) == 5 * n + 4 and all(rng[5 * n:])
    assert [(N[5 * n + i] - base[5 * n + i]) % Q for i in range(7)] == rng[5 * n:] + [0, 0, 0]
    # the definition for unsatisfied inputs: out (X^n - 1) = N modulo X^(4n) - g^(4n) above the top rows' share
    without = dict(polys, q_range=[0] * n)
    assert RM.quotient_blinded(without, ALPHA, BETA, GAMMA) == BM.quotient_blinded({k: v for k, v in polys.items() if k != "q_range"},
                                                                                 ALPHA, BETA, GAMMA)


@pytest.mark.parametrize("m", [0, 1, 2, 4])
def test_q_range_zero_gives_the_existing_models_output(m):
    n = 1 << m
    r = random.Random(100 + m)
    polys = {name: [r.randrange(Q) for _ in range(n)] for name in NAMES if name != "q_range"}
    want = QM.quotient(polys, ALPHA, BETA, GAMMA)
    assert RM.quotient(polys, ALPHA, BETA, GAMMA) == want
    assert RM.quotient(dict(polys, q_range=[0] * n), ALPHA, BETA, GAMMA) == want
    live = dict(polys, q_range=[r.randrange(Q) for _ in range(n)])
    got = RM.quotient(live, ALPHA, BETA, GAMMA)
    assert got != want
    # t is N / (x^n - 1) at points of the coset, from the coefficients by Horner
    zeta, omega = M.omega_of(m + 2), M.omega_of(m)
    for s in (0, 1, 4 * n - 1):
        x = RM.DEFAULT_G * pow(zeta, s, Q) % Q
        v = {name: RM.horner(c, x) for name, c in live.items()}
        nx = RM.numerator(v, RM.horner(live["z"], x * omega % Q), RM.horner(live["a"], x * omega % Q), x, n, ALPHA, BETA, GAMMA)
        assert RM.horner(got, x) * (pow(x, n, Q) - 1) % Q == nx, s
