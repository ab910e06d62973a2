"""CPU: the copy permutation as field elements -- the model of tests/perm_product_model.py, the host entry point
pg_domain_generator, and the property the grand product exists for, on circuits built by the CPU oracle (oracle/composer.c +
oracle/gadgets.c, read-only): z wraps to one over the oracle's own sigma and wire values, and not once a wire value changes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import perm_product_model as M  # noqa: E402


def test_root_of_unity_and_the_model_generator():
    t = (M.Q - 1) >> 32
    assert (M.Q - 1) == t << 32 and t % 2 == 1
    assert M.ROOT_OF_UNITY == pow(7, t, M.Q)
    for m in range(0, 33):
        w = M.omega_of(m)
        assert pow(w, 1 << m, M.Q) == 1 and (m == 0 or pow(w, 1 << (m - 1), M.Q) != 1), m


def test_domain_generator_has_order_exactly_2_pow_m():
    import plonk_gadgets_amd as pg
    from plonk_gadgets_amd import _lib
    for m in range(1, 33):
        w = pg.domain_generator(m)
        assert w.limbs() == M.mont(M.omega_of(m)), m
        x = w.to_int()
        assert pow(x, 1 << m, M.Q) == 1 and pow(x, 1 << (m - 1), M.Q) != 1, m
    assert pg.domain_generator(0).to_int() == 1
    out = _lib.Scalar()
    assert _lib.load().pg_domain_generator(33, C.byref(out)) == 2


def test_default_cosets_are_distinct():
    """k_a H != k_b H for every subgroup H of order 2^m, m <= 32: (k_a / k_b)^(2^32) != 1"""
    import plonk_gadgets_amd as pg
    assert tuple(pg.DEFAULT_K) == M.K
    for a in range(4):
        for b in range(4):
            if a != b:
                assert pow(M.K[a] * pow(M.K[b], -1, M.Q) % M.Q, 1 << 32, M.Q) != 1, (a, b)


def oracle_circuit():
    """a small circuit on the CPU oracle's composer: range_check ladders, max_bound, maybe_equal, is_non_zero, the two selects, a
    boolean gate and constrain_to_constant -- every kind of row the device composer appends"""
    from oracle import pyoracle as po
    from plonk_gadgets_amd import synth
    comp = po.Composer()
    L = comp.L
    f = lambda x: po.fr(synth.mont(x))
    res = []
    for w in (5, 70_000, 249_999):
        res.append(int(L.range_check(comp.c, f(50_000), f(250_000), comp.allocate(synth.mont(w)))))
    a, b = comp.allocate(synth.mont(17)), comp.allocate(synth.mont(17))
    res.append(int(L.max_bound(comp.c, f(300), a, None)))
    res.append(int(L.maybe_equal(comp.c, a, b)))
    assert L.is_non_zero(comp.c, a.var, f(17)) == 0
    one = comp.add_input(synth.mont(1))
    res.append(int(L.conditionally_select_one(comp.c, a.var, one)))
    res.append(int(L.conditionally_select_zero(comp.c, b.var, one)))
    L.composer_boolean_gate(comp.c, one)
    L.composer_constrain_to_constant(comp.c, res[0], f(0), None)
    assert comp.check() == -1
    return comp


def wire_values(comp):
    ex, full = comp.export(), comp.full_columns()
    vals = M.ints_of(ex["var_values"])
    return [[vals[int(v)] for v in ex[name]] for name in ("w_l", "w_r", "w_o")] + [[vals[int(v)] for v in full["w_4"]]]


@pytest.mark.parametrize("extra_log2", [0, 2])
def test_oracle_circuits_wrap_to_one_and_a_changed_value_does_not(extra_log2):
    comp = oracle_circuit()
    n = comp.n
    padded_n = 1 << ((n - 1).bit_length() + extra_log2)
    m = padded_n.bit_length() - 1
    sigma = comp.sigma(padded_n)
    wires = wire_values(comp)
    beta, gamma, omega = 0x1234567 ** 5 % M.Q, 0xABCDEF ** 7 % M.Q, M.omega_of(m)
    z, wrap = M.grand_product(wires, sigma, padded_n, beta, gamma, omega)
    assert z[0] == 1 and wrap == 1 and len(set(z[:64])) > 32
    # the recurrence the definition gives, on every row
    sev = M.sigma_evaluations(sigma, padded_n, omega)
    for i in range(0, padded_n - 1, 97):
        num, den = M.factors(wires, [sev[j][i] for j in range(4)], i, beta, gamma, pow(omega, i, M.Q))
        assert z[i + 1] * den % M.Q == z[i] * num % M.Q
    # one wire value changed in one row (a position on a cycle of more than one): the copy constraints fail
    row = next(i for i in range(3, n) if sigma[0][i] != i)
    bad = [list(w) for w in wires]
    bad[0][row] = (bad[0][row] + 1) % M.Q
    assert M.grand_product(bad, sigma, padded_n, beta, gamma, omega)[1] != 1
    # two sigma entries swapped between positions of different Variables
    ex = comp.export()
    w_l = ex["w_l"]
    i = next(i for i in range(3, n) if sigma[0][i] != i)
    j = next(j for j in range(3, n) if w_l[j] != w_l[i] and sigma[0][j] != j)
    sw = sigma.copy()
    sw[0][i], sw[0][j] = sigma[0][j], sigma[0][i]
    assert M.grand_product(wires, sw, padded_n, beta, gamma, omega)[1] != 1


def test_identity_permutation_and_sigma_evaluations_of_the_identity():
    """sigma = identity: every ratio is one, whatever the wire values; its evaluations are k_j omega^i"""
    padded_n, m = 16, 4
    omega = M.omega_of(m)
    ident = np.arange(4 * padded_n, dtype=np.uint64).reshape(4, padded_n)
    sev = M.sigma_evaluations(ident, padded_n, omega)
    assert sev == [[M.K[j] * pow(omega, i, M.Q) % M.Q for i in range(padded_n)] for j in range(4)]
    wires = [[(7 * i + j) % M.Q for i in range(11)] for j in range(4)]
    z, wrap = M.grand_product(wires, ident, padded_n, 3, 5, omega)
    assert z == [1] * padded_n and wrap == 1
