"""GPU: pg_quotient (csrc/quotient.hpp) through Engine.quotient against the Python-int model of tests/quotient_model.py, limb for limb,
at every n from 2^0 to 2^12 on random inputs and on a composer of every kind of tests/test_gpu_perm_product.py; the identity
t(r) (r^n - 1) = N(r) at a random r through Engine.evaluate, which holds iff the rows and the copy constraints do, and which a changed
Variable value, two swapped sigma entries, a changed public input or a z of another beta break; the error cases of the C ABI; and a
range_check composer padded to 2^28, closed before its quotient is computed."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perm_product_model as PM  # noqa: E402
import quotient_model as QM  # noqa: E402
from test_gpu_perm_product import KINDS as CIRCUITS, build  # noqa: E402

DEV = "cuda:0"
S = pg.BlsScalar.from_int
ALPHA, BETA, GAMMA = 0x5EED_0031 ** 7 % PM.Q, 0x5EED_0032 ** 9 % PM.Q, 0x5EED_0033 ** 11 % PM.Q
R = 0x5EED_0034 ** 13 % PM.Q  # the random evaluation point
NAMES = {"a": ("wires", 0), "b": ("wires", 1), "c": ("wires", 2), "d": ("wires", 3), "z": ("z", None),
         "s1": ("sigmas", 0), "s2": ("sigmas", 1), "s3": ("sigmas", 2), "s4": ("sigmas", 3), "pi": ("pi", None)}


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


def column(polys, name):
    """one input polynomial of a prover_polynomials()-shaped dict by its model name"""
    if name in QM.SELECTORS:
        return polys["selectors"][name]
    key, j = NAMES[name]
    return polys[key] if j is None else polys[key][j]


def model_of(polys):
    """the model's t (ints) for a prover_polynomials()-shaped dict of device tensors"""
    ints = {name: PM.ints_of(host(column(polys, name))) for name in list(NAMES) + list(QM.SELECTORS) if polys.get("pi") is not None
            or name != "pi"}
    return QM.quotient(ints, ALPHA, BETA, GAMMA)


def identity_holds(engine, polys, t):
    """t(r) (r^n - 1) == N(r), every value through Engine.evaluate"""
    n = t.shape[1]
    v = {name: x.to_int() for name, x in zip(NAMES, engine.evaluate(polys["wires"], R) + engine.evaluate(polys["z"], R)
                                                  + engine.evaluate(polys["sigmas"], R) + engine.evaluate(polys["pi"], R))}
    for name in QM.SELECTORS:
        v[name] = engine.evaluate(polys["selectors"][name], R)[0].to_int()
    zw = engine.evaluate(polys["z"], R * PM.omega_of(n.bit_length() - 1) % PM.Q)[0].to_int()
    pieces = [x.to_int() for x in engine.evaluate(t, R)]
    return QM.identity_from_values(v, zw, pieces, R, n, ALPHA, BETA, GAMMA)


def quotient(engine, polys):
    return engine.quotient(**polys, alpha=S(ALPHA), beta=S(BETA), gamma=S(GAMMA))


@pytest.mark.parametrize("m", range(0, 13))
def test_random_inputs_equal_the_model(engine, m):
    n = 1 << m
    x = random_limbs((18, n), seed=300 + m)
    polys = {"wires": x[0:4], "z": x[4], "sigmas": x[5:9], "pi": x[16] if m % 2 else None,
             "selectors": {name: x[9 + i] for i, name in enumerate(QM.SELECTORS)}}
    t = quotient(engine, polys)
    assert t.shape == (4, n, 4)
    assert np.array_equal(host(t).reshape(4 * n, 4), PM.limbs_of(model_of(polys))), m
    # a caller's scratch, and the inputs are left alone
    before = x.clone()
    scratch = torch.full((8, n, 4), -1, dtype=torch.int64, device=DEV)
    assert torch.equal(engine.quotient(**polys, alpha=S(ALPHA), beta=S(BETA), gamma=S(GAMMA), scratch=scratch), t)
    assert torch.equal(x, before)


@pytest.mark.parametrize("circuit", CIRCUITS)
def test_composer_quotient_equals_the_model_and_the_identity_holds_iff_the_circuit_does(engine, circuit):
    comp = build(engine, circuit)
    n = comp.circuit_size()
    padded_n = 1 << (n - 1).bit_length()
    satisfied = comp.check() == -1 and comp.copy_constraints_hold()
    assert satisfied == (circuit != "gate_batches")
    polys = comp.prover_polynomials(S(BETA), S(GAMMA))
    assert polys["wires"].shape == polys["sigmas"].shape == (4, padded_n, 4) and set(polys["selectors"]) == set(QM.SELECTORS)
    assert torch.equal(polys["z"], comp.permutation_polynomial(S(BETA), S(GAMMA)))
    assert torch.equal(polys["wires"], comp.wire_polynomials())
    assert torch.equal(polys["sigmas"], comp.sigma_polynomials())
    t = comp.quotient_polynomial(S(ALPHA), S(BETA), S(GAMMA))
    comp.close()
    assert torch.equal(t, quotient(engine, polys))
    assert identity_holds(engine, polys, t) == satisfied
    if satisfied:
        assert bool((t[3, -4:] == 0).all())
    if padded_n <= 1 << 14:  # (the model's 4n-point transform: up to 2^16 points)
        assert np.array_equal(host(t).reshape(4 * padded_n, 4), PM.limbs_of(model_of(polys))), circuit


def test_corruptions_break_the_identity(engine):
    comp = build(engine, "allocated")
    n = comp.circuit_size()
    padded_n = 1 << (n - 1).bit_length()
    polys = comp.prover_polynomials(S(BETA), S(GAMMA))
    assert identity_holds(engine, polys, quotient(engine, polys))
    # a z built with another beta
    bad = dict(polys, z=comp.permutation_polynomial(S(BETA + 1), S(GAMMA)))
    assert not identity_holds(engine, bad, quotient(engine, bad))
    # one dense public input
    dense = torch.zeros((padded_n, 4), dtype=torch.int64, device=DEV)
    dense[:n] = comp.construct_dense_pi_vec()
    dense[n // 2] = torch.from_numpy(PM.limbs_of([12345]).view(np.int64)).to(DEV)[0]
    bad = dict(polys, pi=engine.ifft(dense))
    assert not identity_holds(engine, bad, quotient(engine, bad))
    # two sigma entries of different Variables swapped
    sigma = comp.permutation(padded_n)
    hs, w_l = host(sigma), host(comp.device_columns().w_l)
    i = next(i for i in range(3, n) if hs[0, i] != i)
    j = next(j for j in range(3, n) if w_l[j] != w_l[i] and hs[0, j] != j)
    sw = sigma.clone()
    sw[0, i], sw[0, j] = sigma[0, j], sigma[0, i]
    comp.permutation = lambda padded_n=None: sw
    bad = comp.prover_polynomials(S(BETA), S(GAMMA))
    del comp.permutation
    assert not identity_holds(engine, bad, quotient(engine, bad))
    # one Variable's value, in the composer's own table
    cols = comp.device_columns()
    q_l = host(cols.q_l)
    v = int(w_l[next(r for r in range(3, n) if q_l[r].any())])
    cols.var_values[v, 0] += 1
    torch.cuda.synchronize()
    assert comp.check() != -1
    bad = comp.prover_polynomials(S(BETA), S(GAMMA))
    assert not identity_holds(engine, bad, quotient(engine, bad))
    cols.var_values[v, 0] -= 1
    torch.cuda.synchronize()
    assert identity_holds(engine, polys, quotient(engine, polys))
    comp.close()


def test_error_cases(engine):
    lib, m = engine._lib, 6
    n = 1 << m
    x = random_limbs((18, n), seed=5)
    t = torch.zeros((4, n, 4), dtype=torch.int64, device=DEV)
    scratch = torch.zeros((8, n, 4), dtype=torch.int64, device=DEV)
    zeta, g, one = pg.domain_generator(m + 2), S(7), S(1)
    ks = (pg._lib.Scalar * 4)(*[S(k).c for k in pg.DEFAULT_K])

    def polys(**over):
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

    def raw(log2_n=m, p=None, omega=zeta, gen=g, d_t=None, d_s=None):
        p = polys() if p is None else p
        return lib.pg_quotient(engine._h, log2_n, C.byref(p), C.byref(S(ALPHA).c), C.byref(S(BETA).c), C.byref(S(GAMMA).c),
                               C.byref(omega.c), ks, C.byref(gen.c), t.data_ptr() if d_t is None else d_t,
                               scratch.data_ptr() if d_s is None else d_s, engine._stream())
    assert raw() == 0 and raw(p=polys(pi=None)) == 0
    ref = t.clone()
    bad = {"log2_n > 30": raw(log2_n=31, omega=pg.domain_generator(32)),
           "omega_4n of order 2n": raw(omega=pg.domain_generator(m + 1)),
           "omega_4n of order 8n": raw(omega=pg.domain_generator(m + 3)),
           "omega_4n = 1": raw(omega=one),
           "g = 0": raw(gen=S(0)),
           "g = 1": raw(gen=one),
           "g in the 4n-th roots": raw(gen=pg.domain_generator(m + 2)),
           "NULL z": raw(p=polys(z=None)),
           "NULL q_arith": raw(p=polys(q_arith=None)),
           "misaligned sigma": raw(p=polys(sigma=(C.c_void_p * 4)(x[5].data_ptr(), x[6].data_ptr() + 8, x[7].data_ptr(), x[8].data_ptr()))),
           "NULL d_t": raw(d_t=0),
           "misaligned scratch": raw(d_s=scratch.data_ptr() + 8),
           "d_t over an input": raw(d_t=x[10].data_ptr()),
           "d_t ending in an input": raw(d_t=x[0].data_ptr() - 3 * n * 32),
           "scratch over pi": raw(d_s=x[12].data_ptr()),
           "d_t over scratch": raw(d_t=scratch.data_ptr() + 32 * n)}
    assert all(st == 2 for st in bad.values()), bad
    assert lib.pg_quotient(engine._h, m, None, C.byref(S(ALPHA).c), C.byref(S(BETA).c), C.byref(S(GAMMA).c), C.byref(zeta.c), ks,
                           C.byref(g.c), t.data_ptr(), scratch.data_ptr(), engine._stream()) == 2
    torch.cuda.synchronize()
    assert torch.equal(t, ref)  # nothing was launched
    # through the Python layer
    p = {"wires": x[0:4], "z": x[4], "sigmas": x[5:9], "selectors": {name: x[9 + i] for i, name in enumerate(QM.SELECTORS)}}
    with pytest.raises(pg.PgError):
        engine.quotient(**p, alpha=1, beta=2, gamma=3, g=1)
    with pytest.raises(ValueError):
        engine.quotient(**dict(p, z=x[4, :n - 1]), alpha=1, beta=2, gamma=3)
    # and the engine goes on
    got = engine.quotient(**p, alpha=S(ALPHA), beta=S(BETA), gamma=S(GAMMA))
    assert np.array_equal(host(got).reshape(4 * n, 4), PM.limbs_of(model_of(dict(p, pi=None))))


def test_full_size_range_check_composer(engine):
    """260 000 x (allocate + range_check(0, 2^254)) = 268 060 003 rows, padded to 2^28: prover_polynomials, the composer closed,
    then the quotient; the identity holds at a random point and the top four coefficients of t_4th are zero"""
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (250 << 30):
        pytest.skip("not enough free HBM for the 2^28 quotient's inputs, scratch and output")
    batch = 260_000
    comp = pg.StandardComposer(engine, 3 + batch * 1031 + 8, 5 + batch * 1034 + 8)
    comp.range_check_batch(S(0), S(2**254), torch.from_numpy(synth.random_scalars(batch, seed=synth.SEED + 9).view(np.int64)).to(DEV))
    n = comp.circuit_size()
    assert n <= 1 << 28 and (1 << (n - 1).bit_length()) == 1 << 28
    assert comp.check() == -1
    polys = comp.prover_polynomials(S(BETA), S(GAMMA))
    comp.close()
    gc.collect()
    t = quotient(engine, polys)
    assert bool((t[3, -4:] == 0).all()) and not bool((t[3, -8:-4] == 0).all())
    assert identity_holds(engine, polys, t)
    del t, polys
    gc.collect()
    torch.cuda.empty_cache()
