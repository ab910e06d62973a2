"""CPU: tests/pairing_model.py pinned by what can be checked without the dependency: the G2 generator is on the twist and of
order r; e(G1, G2) is not 1 and has order r; bilinearity (a = r - 1 included); e(P, Q) e(-P, Q) = 1; the KZG identity of a small
polynomial under a known tau; the Frobenius constants against x -> x^p; the hard part's exponent identity and the device's
addition chain (the cube of the plain power); and the constants embedded in csrc/pairing_constants.inc are what the model
derives."""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import g1_model as G  # noqa: E402
import pairing_model as M  # noqa: E402

P, R = M.P, M.R
E_GH = M.pairing(G.G, M.G2)


def test_generator_is_on_the_twist_and_of_order_r():
    assert M.on_twist(M.G2)
    assert M.g2_mul(R, M.G2) is None
    assert M.g2_mul(R - 1, M.G2) == M.g2_neg(M.G2)
    assert M.g2_compressed(None) == bytes([0xC0]) + bytes(95)
    assert len(M.g2_compressed(M.G2)) == 96 and M.g2_compressed(M.G2)[0] & 0x80


def test_the_pairing_is_not_degenerate_and_has_order_r():
    assert E_GH != M.F12_ONE
    assert M.f12_pow(E_GH, R) == M.F12_ONE


def test_bilinearity():
    for a, b in ((2, 3), (5, 7), (R - 1, 1), (R - 1, R - 1), (0x1234567, 0xFEDCBA987)):
        assert M.pairing(G.mul(a, G.G), M.g2_mul(b, M.G2)) == M.f12_pow(E_GH, a * b % R), (a, b)
    p = G.mul(11, G.G)
    q = M.g2_mul(13, M.G2)
    assert M.f12_mul(M.pairing(p, q), M.pairing(G.neg(p), q)) == M.F12_ONE


def test_field_tower():
    rng = random.Random(12)
    f = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
    g = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
    assert M.f12_mul(f, M.f12_inv(f)) == M.F12_ONE
    assert M.f12_mul(f, g) == M.f12_mul(g, f)
    assert M.f12_frobenius(f, 1) == M.f12_pow(f, P)
    assert M.f12_frobenius(f, 2) == M.f12_pow(f, P * P)
    assert M.f12_frobenius(f, 3) == M.f12_pow(f, P ** 3)
    assert M.f12_conj(f) == M.f12_pow(f, P ** 6)
    assert all(c[1] == 0 for c in M.GAMMA2)
    w = [(0, 0), (1, 0)] + [(0, 0)] * 4
    assert M.f12_pow(w, 6) == [M.XI] + [(0, 0)] * 5
    a = (rng.randrange(P), rng.randrange(P))
    assert M.f2_sqr(M.f2_sqrt(M.f2_sqr(a))) == M.f2_sqr(a)
    assert M.f2_mul(a, M.f2_inv(a)) == (1, 0) and M.f2_inv((0, 0)) == (0, 0)


def test_the_final_exponentiation_chain_is_the_cube_of_the_plain_power():
    x = -M.X_ABS
    assert (P ** 4 - P ** 2 + 1) % R == 0
    assert M.HARD_C * ((P ** 4 - P ** 2 + 1) // R) == (x - 1) ** 2 * (x + P) * (x * x + P * P - 1) + 3
    assert (P ** 12 - 1) // R == (P ** 6 - 1) * (P ** 2 + 1) * ((P ** 4 - P ** 2 + 1) // R)
    f = M.miller_loop([(G.mul(3, G.G), M.g2_prepare(M.g2_mul(5, M.G2)))])
    assert M.final_exponentiation_chain(f) == M.f12_pow(M.final_exponentiation_plain(f), M.HARD_C)
    assert len(M.g2_prepare(M.G2)) == M.N_LINES == 68


def test_kzg_identity_under_a_known_tau():
    """f = 3 + 2 X + X^3 opened at z: e([f(tau) - f(z)]_1, [1]_2) = e([q(tau)]_1, [tau - z]_2), and as the two-pair product the
    verifier checks; a wrong value fails"""
    tau, z = 0xDECAF, 0xBEEF
    f = lambda x: (3 + 2 * x + x ** 3) % R  # noqa: E731
    q_tau = (f(tau) - f(z)) * pow(tau - z, -1, R) % R
    w = G.mul(q_tau, G.G)
    lhs = M.pairing(w, M.g2_mul((tau - z) % R, M.G2))
    assert lhs == M.pairing(G.mul((f(tau) - f(z)) % R, G.G), M.G2)
    h, tau_h = M.g2_prepare(M.G2), M.g2_prepare(M.g2_mul(tau, M.G2))

    def check(value):
        other = G.neg(G.add(G.mul(z, w), G.mul((f(tau) - value) % R, G.G)))
        return M.final_exponentiation_plain(M.miller_loop([(w, tau_h), (other, h)])) == M.F12_ONE
    assert check(f(z)) and not check((f(z) + 1) % R)


def test_embedded_constants_are_the_models():
    import gen_pairing_constants as gen
    path = os.path.join(ROOT, "plonk_gadgets_amd", "csrc", "pairing_constants.inc")
    assert open(path).read() == gen.generate(), "run python tools/gen_pairing_constants.py"
