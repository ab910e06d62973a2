"""GPU: pg_quotient_blinded (csrc/quotient.hpp) through Engine.quotient_blinded against the Python-int model of
tests/quotient_blinded_model.py, limb for limb: at every n from 2^3 (the floor) to 2^10 and at 2^12 on random inputs -- random
tails, so N is not divisible and the target is the definition for arbitrary inputs -- with and without pi; on a composer of every
append kind of tests/test_gpu_perm_product.py at its natural padded size, blinded with random scalars, where the identity
t(r) (r^n - 1) = N(r) also holds at a random r through Engine.evaluate on the 4n + 8 column iff the circuit is satisfied; with tails
of zero rows 0..4n-1 are Engine.quotient's and rows 4n..4n+7 zero; a sentinel row behind d_t and behind each input survives; and
the error cases of the C ABI launch nothing."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perm_product_model as PM  # noqa: E402
import quotient_blinded_model as BM  # noqa: E402
import quotient_model as QM  # noqa: E402
from test_gpu_perm_product import KINDS as CIRCUITS, build  # noqa: E402

DEV = "cuda:0"
S = pg.BlsScalar.from_int
ALPHA, BETA, GAMMA = 0x5EED_0051 ** 7 % PM.Q, 0x5EED_0052 ** 9 % PM.Q, 0x5EED_0053 ** 11 % PM.Q
R = 0x5EED_0054 ** 13 % PM.Q  # the random evaluation point
SENTINEL = -0x0123456789ABCDEF
MODEL_MAX_N = 1 << 13  # the model's 8n-point transform: up to 2^16 points


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def random_limbs(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2**64, size=shape + (4,), dtype=np.uint64)
    x[..., 3] %= np.uint64(0x73EDA753299D7D48)
    return torch.from_numpy(x.view(np.int64)).to(DEV)


def random_inputs(n, seed, with_pi):
    """18 columns of n + 4 rows: the wires use n + 2 of them, z n + 3, the rest n; the row behind each is a sentinel"""
    x = random_limbs((18, n + 4), seed)
    rows = [n + 2] * 4 + [n + 3] + [n] * 13
    for i, r in enumerate(rows):
        x[i, r:] = SENTINEL
    polys = {"wires": [x[j, :n + 2] for j in range(4)], "z": x[4, :n + 3], "sigmas": [x[5 + j, :n] for j in range(4)],
             "pi": x[16, :n] if with_pi else None, "selectors": {name: x[9 + i, :n] for i, name in enumerate(QM.SELECTORS)}}
    return x, rows, polys


def model_of(polys):
    """the model's 4n + 8 ints for a quotient_blinded()-shaped dict of device tensors"""
    ints = {name: PM.ints_of(host(polys["wires"][j])) for j, name in enumerate(BM.WIRES)}
    ints["z"] = PM.ints_of(host(polys["z"]))
    for j in range(4):
        ints["s%d" % (j + 1)] = PM.ints_of(host(polys["sigmas"][j]))
    for name in QM.SELECTORS:
        ints[name] = PM.ints_of(host(polys["selectors"][name]))
    if polys.get("pi") is not None:
        ints["pi"] = PM.ints_of(host(polys["pi"]))
    return BM.quotient_blinded(ints, ALPHA, BETA, GAMMA)


def quotient_blinded(engine, polys, **kw):
    return engine.quotient_blinded(**polys, alpha=S(ALPHA), beta=S(BETA), gamma=S(GAMMA), **kw)


@pytest.mark.parametrize("m", list(range(3, 11)) + [12])
def test_random_inputs_equal_the_model(engine, m):
    n = 1 << m
    x, rows, polys = random_inputs(n, seed=500 + m, with_pi=bool(m % 2))
    before = x.clone()
    t = quotient_blinded(engine, polys)
    assert t.shape == (4 * n + 8, 4)
    assert np.array_equal(host(t), PM.limbs_of(model_of(polys))), m
    assert bool((t[4 * n + 7] == 0).all()) and bool((t[4 * n:4 * n + 7] != 0).any())
    assert torch.equal(x, before)  # the inputs, and the row behind each, are left alone
    # the other setting of pi at the two ends, against the same model
    if m in (3, 10):
        other = dict(polys, pi=None if polys["pi"] is not None else x[16, :n])
        assert np.array_equal(host(quotient_blinded(engine, other)), PM.limbs_of(model_of(other))), m


def raw_call(engine, log2_n, p, d_t, d_s, omega=None, gen=None):
    ks = (pg._lib.Scalar * 4)(*[S(k).c for k in pg.DEFAULT_K])
    omega = pg.domain_generator(log2_n + 2) if omega is None else omega
    gen = S(7) if gen is None else gen
    return engine._lib.pg_quotient_blinded(engine._h, log2_n, None if p is None else C.byref(p), C.byref(S(ALPHA).c),
                                           C.byref(S(BETA).c), C.byref(S(GAMMA).c), C.byref(omega.c), ks, C.byref(gen.c), d_t, d_s,
                                           engine._stream())


def polys_c(x, n, **over):
    p = pg._lib.QuotientPolysC()
    for j in range(4):
        p.w[j] = x[j].data_ptr()
        p.sigma[j] = x[5 + j].data_ptr()
    p.z = x[4].data_ptr()
    for i, name in enumerate(QM.SELECTORS):
        setattr(p, name, x[9 + i].data_ptr())
    p.pi = x[16].data_ptr()
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("m", [3, 6, 11])
def test_sentinels_behind_the_output_the_scratch_and_the_inputs_survive(engine, m):
    n = 1 << m
    x, rows, polys = random_inputs(n, seed=600 + m, with_pi=True)
    before = x.clone()
    t = torch.full((4 * n + 9, 4), SENTINEL, dtype=torch.int64, device=DEV)
    scratch = torch.full((8 * n + 1, 4), SENTINEL, dtype=torch.int64, device=DEV)
    assert raw_call(engine, m, polys_c(x, n), t.data_ptr(), scratch.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((t[4 * n + 8] == SENTINEL).all()) and bool((scratch[8 * n] == SENTINEL).all())
    assert torch.equal(x, before)
    assert torch.equal(t[:4 * n + 8], quotient_blinded(engine, polys))


@pytest.mark.parametrize("m", [3, 5, 11])
def test_zero_tails_give_the_unblinded_quotient_and_eight_zero_rows(engine, m):
    n = 1 << m
    x, rows, polys = random_inputs(n, seed=700 + m, with_pi=bool(m % 2))
    for j in range(5):
        x[j, n:rows[j]] = 0
    plain = dict(polys, wires=[x[j, :n] for j in range(4)], z=x[4, :n])
    want = engine.quotient(**plain, alpha=S(ALPHA), beta=S(BETA), gamma=S(GAMMA))
    t = quotient_blinded(engine, polys)
    assert torch.equal(t[:4 * n], want.reshape(4 * n, 4))
    assert bool((t[4 * n:] == 0).all())


def blinded_polys(engine, comp, seed):
    """prover_polynomials(tail=8) of the composer, blinded with 11 random scalars, as quotient_blinded()'s arguments; and the
    full tail-padded columns"""
    n = comp.circuit_size()
    padded_n = 1 << (n - 1).bit_length()
    pp = comp.prover_polynomials(S(BETA), S(GAMMA), tail=8)
    assert pp["wires"].shape == (4, padded_n + 8, 4) and pp["z"].shape == (padded_n + 8, 4)
    assert bool((pp["wires"][:, padded_n:] == 0).all()) and bool((pp["z"][padded_n:] == 0).all())
    plain = comp.prover_polynomials(S(BETA), S(GAMMA))
    assert torch.equal(pp["wires"][:, :padded_n], plain["wires"]) and torch.equal(pp["z"][:padded_n], plain["z"])
    r = random.Random(seed)
    b = [r.randrange(PM.Q) for _ in range(11)]
    for j in range(4):
        engine.blind(pp["wires"][j], padded_n, b[2 * j:2 * j + 2])
    engine.blind(pp["z"], padded_n, b[8:11])
    # Engine.blind is the model's blind
    assert PM.ints_of(host(pp["z"][:padded_n + 3])) == BM.blind(PM.ints_of(host(plain["z"])), padded_n, b[8:11])
    assert PM.ints_of(host(pp["wires"][2, :padded_n + 2])) == BM.blind(PM.ints_of(host(plain["wires"][2])), padded_n, b[4:6])
    assert bool((pp["wires"][:, padded_n + 2:] == 0).all()) and bool((pp["z"][padded_n + 3:] == 0).all())
    args = dict(pp, wires=[pp["wires"][j, :padded_n + 2] for j in range(4)], z=pp["z"][:padded_n + 3])
    return padded_n, pp, args


def identity_holds(engine, pp, t, n):
    """t(r) (r^n - 1) == N(r): every value through Engine.evaluate, t as ONE column of 4n + 8 coefficients"""
    names = list(BM.WIRES) + ["z", "s1", "s2", "s3", "s4", "pi"]
    vals = engine.evaluate(pp["wires"], R) + engine.evaluate(pp["z"], R) + engine.evaluate(pp["sigmas"], R) + engine.evaluate(pp["pi"], R)
    v = {name: x.to_int() for name, x in zip(names, vals)}
    for name in QM.SELECTORS:
        v[name] = engine.evaluate(pp["selectors"][name], R)[0].to_int()
    zw = engine.evaluate(pp["z"], R * PM.omega_of(n.bit_length() - 1) % PM.Q)[0].to_int()
    t_r = engine.evaluate(t, R)[0].to_int()
    return t_r * (pow(R, n, PM.Q) - 1) % PM.Q == QM.numerator(v, zw, R, n, ALPHA, BETA, GAMMA)


@pytest.mark.parametrize("circuit", CIRCUITS)
def test_composer_quotient_equals_the_model_and_the_identity_holds_iff_the_circuit_does(engine, circuit):
    comp = build(engine, circuit)
    satisfied = comp.check() == -1 and comp.copy_constraints_hold()
    assert satisfied == (circuit != "gate_batches")
    padded_n, pp, args = blinded_polys(engine, comp, seed=circuit)
    comp.close()
    t = quotient_blinded(engine, args)
    assert t.shape == (4 * padded_n + 8, 4)
    assert identity_holds(engine, pp, t, padded_n) == satisfied
    assert bool((t[4 * padded_n + 7] == 0).all())
    if satisfied:  # random blinders: the quotient reaches degree 4n + 6
        assert bool((t[4 * padded_n + 6] != 0).any())
    if padded_n <= MODEL_MAX_N:
        assert np.array_equal(host(t), PM.limbs_of(model_of(args))), circuit


def test_error_cases(engine):
    m = 6
    n = 1 << m
    x, rows, polys = random_inputs(n, seed=5, with_pi=True)
    t = torch.zeros((4 * n + 8, 4), dtype=torch.int64, device=DEV)
    scratch = torch.zeros((8, n, 4), dtype=torch.int64, device=DEV)
    one = S(1)

    def raw(log2_n=m, p=False, d_t=None, d_s=None, **kw):
        p = polys_c(x, n) if p is False else p
        return raw_call(engine, log2_n, p, t.data_ptr() if d_t is None else d_t, scratch.data_ptr() if d_s is None else d_s, **kw)
    assert raw() == 0 and raw(p=polys_c(x, n, pi=None)) == 0
    torch.cuda.synchronize()
    ref = t.clone()
    row = 32
    # a wire (n + 2 rows) or z (n + 3) directly in front of, or behind, a d_t of 4n + 8 rows, in buffers of their own: only the
    # longer extents tell the cases that touch from the cases that overlap
    front = torch.zeros((n + 3 + 4 * n + 8, 4), dtype=torch.int64, device=DEV)
    back = torch.zeros((4 * n + 8 + n + 3, 4), dtype=torch.int64, device=DEV)
    w_front = (C.c_void_p * 4)(front.data_ptr(), x[1].data_ptr(), x[2].data_ptr(), x[3].data_ptr())
    bad = {"log2_n = 2": raw(log2_n=2),
           "log2_n > 30": raw(log2_n=31, omega=pg.domain_generator(32)),
           "NULL p": raw(p=None),
           "NULL z": raw(p=polys_c(x, n, z=None)),
           "misaligned z": raw(p=polys_c(x, n, z=x[4].data_ptr() + 8)),
           "omega_4n of order 2n": raw(omega=pg.domain_generator(m + 1)),
           "omega_4n of order 8n": raw(omega=pg.domain_generator(m + 3)),
           "g = 0": raw(gen=S(0)),
           "g = 1": raw(gen=one),
           "g in the 4n-th roots": raw(gen=pg.domain_generator(m + 2)),
           "NULL d_t": raw(d_t=0),
           "misaligned scratch": raw(d_s=scratch.data_ptr() + 8),
           "d_t over a wire's two tail rows": raw(p=polys_c(x, n, w=w_front), d_t=front.data_ptr() + n * row),
           "d_t over a wire's second tail row": raw(p=polys_c(x, n, w=w_front), d_t=front.data_ptr() + (n + 1) * row),
           "d_t over z's third tail row": raw(p=polys_c(x, n, z=front.data_ptr()), d_t=front.data_ptr() + (n + 2) * row),
           "d_t's row 4n + 7 over z": raw(p=polys_c(x, n, z=back.data_ptr() + (4 * n + 7) * row), d_t=back.data_ptr()),
           "d_t's row 4n over q_c": raw(p=polys_c(x, n, q_c=back.data_ptr() + 4 * n * row), d_t=back.data_ptr()),
           "d_t over scratch": raw(d_t=scratch.data_ptr() + row * n)}
    assert all(st == 2 for st in bad.values()), bad
    torch.cuda.synchronize()
    assert torch.equal(t, ref)  # nothing was launched
    # touching is fine: d_t right behind a wire's two tail rows, behind z's three, and z right behind d_t's 4n + 8 rows
    assert raw(p=polys_c(x, n, w=w_front), d_t=front.data_ptr() + (n + 2) * row) == 0
    assert raw(p=polys_c(x, n, z=front.data_ptr()), d_t=front.data_ptr() + (n + 3) * row) == 0
    assert raw(p=polys_c(x, n, z=back.data_ptr() + (4 * n + 8) * row), d_t=back.data_ptr()) == 0
    torch.cuda.synchronize()
    # through the Python layer
    with pytest.raises(pg.PgError):
        quotient_blinded(engine, polys, g=1)
    with pytest.raises(ValueError):
        quotient_blinded(engine, dict(polys, z=x[4, :n + 2]))
    with pytest.raises(ValueError):
        quotient_blinded(engine, dict(polys, wires=[x[j, :n] for j in range(4)]))
    small = random_inputs(4, seed=6, with_pi=False)[2]
    with pytest.raises(ValueError):
        quotient_blinded(engine, small)
    with pytest.raises(ValueError):
        engine.blind(x[0, :n + 1], n, [1, 2])
    # and the engine goes on
    assert np.array_equal(host(quotient_blinded(engine, polys)), PM.limbs_of(model_of(polys)))
