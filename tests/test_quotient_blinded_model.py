"""CPU: the blinded-quotient model of tests/quotient_blinded_model.py on circuits built by the CPU oracle (oracle/composer.c +
oracle/gadgets.c, read-only; the builders of tests/test_quotient_model.py and tests/test_perm_product_model.py) with a public input
and random blinders, padded to n = 8, 16, 32 and 64 (8 is the derived floor: the blinders' low rows 0..2 and the top windows, down
to row n - 5, do not meet): the division by X^n - 1 leaves no remainder, deg t <= 4n + 6, the definition for arbitrary inputs
equals the exact quotient, t(xi) Z_H(xi) = N(xi) at a random xi, a changed wire value breaks all of that, and with blinders of
zero the result is tests/quotient_model.py's t with eight zero rows behind it.  On random (unsatisfied) inputs the definition's T_i
are the schoolbook coefficients 5n + i of N."""
import ctypes as C
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
from test_perm_product_model import wire_values  # noqa: E402
from test_quotient_model import ALPHA, BETA, GAMMA, PI, polys_of  # noqa: E402

XI = 0x5EED_0041 ** 13 % M.Q
SIZES = [8, 16, 32, 64]


def small_circuit(padded_n: int):
    """an oracle circuit of the scalar gadgets and a public input whose size pads to padded_n; at 8 and 32 it is exactly padded_n
    rows (no spare rows), at 16 and 64 it is not"""
    from oracle import pyoracle as po
    from plonk_gadgets_amd import synth
    comp = po.Composer()
    L = comp.L
    f = lambda x: po.fr(synth.mont(x))
    a, b = comp.allocate(synth.mont(17)), comp.allocate(synth.mont(17))
    one = comp.add_input(synth.mont(1))
    L.composer_constrain_to_constant(comp.c, a.var, f(17 + PI), C.byref(f(PI)))
    L.maybe_equal(comp.c, a, b)
    want = padded_n if padded_n in (8, 32) else padded_n - 3
    i = 0
    while comp.n + 4 <= want:
        (L.conditionally_select_one if i % 2 else L.conditionally_select_zero)(comp.c, a.var, one)
        i += 1
    if comp.n + 3 <= want:
        assert L.is_non_zero(comp.c, a.var, f(17)) == 0
    while comp.n < want:
        L.composer_boolean_gate(comp.c, one)
    assert comp.check() == -1
    assert comp.n == want and 1 << (comp.n - 1).bit_length() == padded_n, (comp.n, padded_n)
    return comp


def blinders(seed):
    r = random.Random(seed)
    return [r.randrange(M.Q) for _ in range(11)]


@pytest.mark.parametrize("n", SIZES)
def test_satisfied_circuit_with_random_blinders(n):
    comp = small_circuit(n)
    base = polys_of(comp)
    assert len(base["z"]) == n and any(base["pi"])
    polys = BM.blind_all(base, blinders(n))
    assert all(len(polys[w]) == n + 2 for w in BM.WIRES) and len(polys["z"]) == n + 3
    # blinding changes no value on H
    omega = M.omega_of(n.bit_length() - 1)
    for name in ("a", "z"):
        assert all(BM.horner(polys[name], pow(omega, i, M.Q)) == BM.horner(base[name], pow(omega, i, M.Q)) for i in (0, 1, n - 1))
    t, rem, deg = BM.exact_quotient(polys, ALPHA, BETA, GAMMA)
    assert not any(rem)
    assert 4 * n <= deg <= 4 * n + 6  # (random blinders: the bound is reached, so the seven extra rows are needed)
    assert len(t) == 4 * n + 8 and t[4 * n + 7] == 0
    assert BM.quotient_blinded(polys, ALPHA, BETA, GAMMA) == t
    lhs, rhs = BM.evaluate_at(polys, t, XI, ALPHA, BETA, GAMMA)
    assert lhs == rhs
    # the 4n-point interpolant alone is NOT the quotient
    assert QM_interpolant(polys) != t[:4 * n]


def QM_interpolant(polys):
    """t~: the degree-< 4n interpolant of N / (x^n - 1) on the coset, by tests/quotient_model.py's own pointwise formula"""
    n = len(polys["s1"])
    zeta = M.omega_of(n.bit_length() + 1)
    ev = {name: BM.coset_fft(list(c) + [0] * (4 * n - len(c)), BM.DEFAULT_G, zeta) for name, c in polys.items()}
    out, x = [], BM.DEFAULT_G
    for i in range(4 * n):
        v = {name: e[i] for name, e in ev.items()}
        out.append(QM.numerator(v, ev["z"][(i + 4) % (4 * n)], x, n, ALPHA, BETA, GAMMA) * pow(pow(x, n, M.Q) - 1, -1, M.Q) % M.Q)
        x = x * zeta % M.Q
    return BM.coset_ifft(out, BM.DEFAULT_G, zeta)


@pytest.mark.parametrize("n", SIZES)
def test_the_definition_folds_the_interpolant(n):
    """out[k] = t~[k] - g^(4n) T_k below 7 and t~[k] elsewhere, with t~ computed as tests/quotient_model.py computes it"""
    polys = BM.blind_all(polys_of(small_circuit(n)), blinders(100 + n))
    out = BM.quotient_blinded(polys, ALPHA, BETA, GAMMA)
    tt, g4n = QM_interpolant(polys), pow(BM.DEFAULT_G, 4 * n, M.Q)
    assert out[7:4 * n] == tt[7:]
    assert all(out[k] == (tt[k] - g4n * out[4 * n + k]) % M.Q for k in range(7))


@pytest.mark.parametrize("n", SIZES)
def test_a_changed_wire_value_breaks_it(n):
    comp = small_circuit(n)
    wires = wire_values(comp)
    sigma = comp.sigma(n)
    row = next(i for i in range(3, comp.n) if sigma[0][i] != i)
    wires[0][row] = (wires[0][row] + 1) % M.Q
    polys = BM.blind_all(polys_of(comp, wires=wires), blinders(200 + n))
    t, rem, _ = BM.exact_quotient(polys, ALPHA, BETA, GAMMA)
    assert any(rem)
    out = BM.quotient_blinded(polys, ALPHA, BETA, GAMMA)
    for cand in (t, out):
        lhs, rhs = BM.evaluate_at(polys, cand, XI, ALPHA, BETA, GAMMA)
        assert lhs != rhs


@pytest.mark.parametrize("n", SIZES)
def test_zero_blinders_give_the_unblinded_quotient_and_eight_zero_rows(n):
    base = polys_of(small_circuit(n))
    polys = BM.blind_all(base, [0] * 11)
    assert polys["a"] == base["a"] + [0, 0] and polys["z"] == base["z"] + [0, 0, 0]
    want = QM.quotient(base, ALPHA, BETA, GAMMA) + [0] * 8
    assert BM.quotient_blinded(polys, ALPHA, BETA, GAMMA) == want
    assert BM.exact_quotient(polys, ALPHA, BETA, GAMMA)[0] == want


@pytest.mark.parametrize("n", [8, 16])
def test_random_inputs_top_coefficients_are_the_schoolbook_ones(n):
    r = random.Random(n)
    names = ["s1", "s2", "s3", "s4"] + list(QM.SELECTORS) + ["pi"]
    polys = {name: [r.randrange(M.Q) for _ in range(n)] for name in names}
    for w in BM.WIRES:
        polys[w] = [r.randrange(M.Q) for _ in range(n + 2)]
    polys["z"] = [r.randrange(M.Q) for _ in range(n + 3)]
    N = BM.numerator_poly(polys, n, ALPHA, BETA, GAMMA)
    assert len(N) == 5 * n + 7 and N[-1]
    out = BM.quotient_blinded(polys, ALPHA, BETA, GAMMA)
    assert out[4 * n:] == N[5 * n:] + [0]
    assert BM.numerator_coefficients(polys, ALPHA, BETA, GAMMA)[:5 * n + 7] == N
    # not divisible: no exact quotient, and the identity fails off the coset
    assert any(BM.divide_by_vanishing(N, n)[1])
    lhs, rhs = BM.evaluate_at(polys, out, XI, ALPHA, BETA, GAMMA)
    assert lhs != rhs
