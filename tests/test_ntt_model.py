"""CPU: the NTT model of tests/ntt_model.py -- its two forms agree, the inverse kinds invert the forward ones, the coset transform
evaluates at g omega^j, omega is the library's and the permutation model's, and the host helper of the full-size GPU test checks the
random-point identity."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ntt_model as M  # noqa: E402
import perm_product_model as PM  # noqa: E402


def rand(n, seed):
    r = random.Random(seed)
    return [r.randrange(M.Q) for _ in range(n)]


@pytest.mark.parametrize("m", range(0, 9))
def test_naive_and_radix2_agree(m):
    c = rand(1 << m, m)
    om = M.omega_of(m)
    assert M.dft(c, om) == M.ntt(c, om)
    assert M.dft(c, pow(om, -1, M.Q)) == M.ntt(c, pow(om, -1, M.Q))


@pytest.mark.parametrize("m", [0, 1, 2, 5, 8, 9, 12])
def test_inverse_kinds_invert(m):
    c = rand(1 << m, 100 + m)
    assert M.ifft(M.fft(c)) == c
    assert M.fft(M.ifft(c)) == c
    assert M.coset_ifft(M.coset_fft(c)) == c
    assert M.coset_ifft(M.coset_fft(c, g=5), g=5) == c


@pytest.mark.parametrize("m", [0, 1, 3, 6, 10])
def test_transforms_evaluate_the_polynomial(m):
    n = 1 << m
    c = rand(n, 200 + m)
    om = M.omega_of(m)
    e, ce = M.fft(c), M.coset_fft(c)
    for j in sorted({j for j in (0, 1, n // 2, n - 1) if j < n} | set(random.Random(m).sample(range(n), min(n, 6)))):
        assert e[j] == M.horner(c, pow(om, j, M.Q))
        assert ce[j] == M.horner(c, M.DEFAULT_G * pow(om, j, M.Q) % M.Q)


def test_special_inputs():
    n = 64
    assert M.fft([0] * n) == [0] * n
    assert M.fft([1] + [0] * (n - 1)) == [1] * n        # a constant polynomial
    assert M.ifft([5] * n) == [5] + [0] * (n - 1)
    om = M.omega_of(6)
    assert M.fft([0, 1] + [0] * (n - 2)) == [pow(om, j, M.Q) for j in range(n)]
    c = [M.Q - 1] * n
    assert M.ifft(M.fft(c)) == c


def test_omega_agrees_with_the_library_and_the_permutation_model():
    import plonk_gadgets_amd as pg
    for m in (0, 1, 2, 10, 16, 29, 31, 32):
        om = M.omega_of(m)
        assert om == PM.omega_of(m) == pg.domain_generator(m).to_int()
        assert pow(om, 1 << m, M.Q) == 1 and (m == 0 or pow(om, 1 << (m - 1), M.Q) == M.Q - 1)
    assert pg.DEFAULT_COSET_GENERATOR == M.DEFAULT_G == 7


@pytest.mark.parametrize("m", [4, 12, 16])
def test_point_identity(m):
    c = rand(1 << m, 300 + m)
    om = M.omega_of(m)
    e = M.fft(c)
    s = 0x5EED_0003 ** 7 % M.Q
    assert M.point_identity_holds(c, e, s, om)
    e[3] = (e[3] + 1) % M.Q
    assert not M.point_identity_holds(c, e, s, om)


def test_host_point_check_helper(tmp_path):
    fn = M.build_point_check(str(tmp_path))
    m = 12
    c = rand(1 << m, 400)
    e = M.fft(c)
    s, om = 0x5EED_0004 ** 5 % M.Q, M.omega_of(m)
    ca, ea = PM.limbs_of(c), PM.limbs_of(e)
    sa, oa = np.array(PM.mont(s), dtype=np.uint64), np.array(PM.mont(om), dtype=np.uint64)
    call = lambda x, y, th: fn(x.ctypes.data, y.ctypes.data, 1 << m, sa.ctypes.data, oa.ctypes.data, th)
    for threads in (1, 3, 16):
        assert call(ca, ea, threads) == 1
    bad = ea.copy()
    bad[77, 0] ^= 1
    assert call(ca, bad, M.point_check_threads()) == 0
    one = np.array(PM.mont(1), dtype=np.uint64)  # s = 1 lies in the subgroup
    assert fn(ca.ctypes.data, ea.ctypes.data, 1 << m, one.ctypes.data, oa.ctypes.data, 4) == -1


@pytest.mark.parametrize("g", [1, 7])
def test_host_point_check_scaled_helper(tmp_path, g):
    """ntt_point_check_scaled against point_identity_holds on c_i g^i, at n = 2^10: a true pair and a spoiled one"""
    fn = M.build_point_check_scaled(str(tmp_path))
    m = 10
    c = rand(1 << m, 500 + g)
    e = M.coset_fft(c, g)
    s, om = 0x5EED_0007 ** 5 % M.Q, M.omega_of(m)
    scaled = [ci * pow(g, i, M.Q) % M.Q for i, ci in enumerate(c)]
    assert M.point_identity_holds(scaled, e, s, om)
    ca, ea = PM.limbs_of(c), PM.limbs_of(e)
    sa, oa, ga = (np.array(PM.mont(v), dtype=np.uint64) for v in (s, om, g))
    call = lambda x, y, th: fn(x.ctypes.data, y.ctypes.data, 1 << m, sa.ctypes.data, oa.ctypes.data, ga.ctypes.data, th)
    for threads in (1, 3, 16):
        assert call(ca, ea, threads) == 1
    for where in (0, 77, (1 << m) - 1):  # one limb of one element, of either array
        bad = ea.copy()
        bad[where, 1] ^= 1 << 17
        spoiled = PM.ints_of(bad)
        assert not M.point_identity_holds(scaled, spoiled, s, om)
        assert call(ca, bad, M.point_check_threads()) == 0
        bad = ca.copy()
        bad[where, 0] ^= 1
        assert call(bad, ea, 5) == 0
    if g != 1:  # the scaling matters: the plain identity does not hold for the coset transform
        one = np.array(PM.mont(1), dtype=np.uint64)
        assert fn(ca.ctypes.data, ea.ctypes.data, 1 << m, sa.ctypes.data, oa.ctypes.data, one.ctypes.data, 4) == 0
        assert M.build_point_check(str(tmp_path))(ca.ctypes.data, ea.ctypes.data, 1 << m, sa.ctypes.data, oa.ctypes.data, 4) == 0
    else:
        assert M.build_point_check(str(tmp_path))(ca.ctypes.data, ea.ctypes.data, 1 << m, sa.ctypes.data, oa.ctypes.data, 4) == 1
