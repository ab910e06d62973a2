"""GPU: pg_quotient_range (csrc/quotient.hpp) through Engine.quotient / Engine.quotient_blinded(q_range=...)
against the Python-int model of tests/quotient_range_model.py, limb for limb, on random inputs with a random q_range: at every n
from 2^1 to 2^10 unblinded and from 2^3 to 2^10 blinded with random tails; with a NULL q_range the bytes are those of pg_quotient /
pg_quotient_blinded; sentinel rows behind d_t, the scratch, q_range and the other inputs survive; an overlap with q_range is
refused with nothing launched."""
import ctypes as C
import os
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
import quotient_range_model as RM  # noqa: E402

DEV = "cuda:0"
S = pg.BlsScalar.from_int
ALPHA, BETA, GAMMA = 0x5EED_0061 ** 7 % PM.Q, 0x5EED_0062 ** 9 % PM.Q, 0x5EED_0063 ** 11 % PM.Q
SENTINEL = -0x0123456789ABCDEF
Q_RANGE = 17  # its column among the inputs


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def random_inputs(n, seed, with_pi, blinded):
    """18 columns of n + 4 rows: blinded, the wires use n + 2 of them and z n + 3, everything else n; behind each, sentinels"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 2**64, size=(18, n + 4, 4), dtype=np.uint64)
    raw[..., 3] %= np.uint64(0x73EDA753299D7D48)
    x = torch.from_numpy(raw.view(np.int64)).to(DEV)
    rows = ([n + 2] * 4 + [n + 3] if blinded else [n] * 5) + [n] * 13
    for i, r in enumerate(rows):
        x[i, r:] = SENTINEL
    polys = {"wires": [x[j, :rows[j]] for j in range(4)], "z": x[4, :rows[4]], "sigmas": [x[5 + j, :n] for j in range(4)],
             "pi": x[16, :n] if with_pi else None, "selectors": {name: x[9 + i, :n] for i, name in enumerate(QM.SELECTORS)},
             "q_range": x[Q_RANGE, :n]}
    return x, polys


def ints_of(polys):
    ints = {name: PM.ints_of(host(polys["wires"][j])) for j, name in enumerate(BM.WIRES)}
    ints["z"] = PM.ints_of(host(polys["z"]))
    for j in range(4):
        ints["s%d" % (j + 1)] = PM.ints_of(host(polys["sigmas"][j]))
    for name in QM.SELECTORS:
        ints[name] = PM.ints_of(host(polys["selectors"][name]))
    if polys.get("pi") is not None:
        ints["pi"] = PM.ints_of(host(polys["pi"]))
    if polys.get("q_range") is not None:
        ints["q_range"] = PM.ints_of(host(polys["q_range"]))
    return ints


def call(engine, polys, blinded, **kw):
    fn = engine.quotient_blinded if blinded else engine.quotient
    return fn(**polys, alpha=S(ALPHA), beta=S(BETA), gamma=S(GAMMA), **kw)


@pytest.mark.parametrize("m", range(1, 11))
def test_unblinded_random_inputs_equal_the_model(engine, m):
    n = 1 << m
    x, polys = random_inputs(n, seed=800 + m, with_pi=bool(m % 2), blinded=False)
    before = x.clone()
    t = call(engine, polys, False)
    assert t.shape == (4, n, 4)
    assert np.array_equal(host(t).reshape(4 * n, 4), PM.limbs_of(RM.quotient(ints_of(polys), ALPHA, BETA, GAMMA))), m
    assert torch.equal(x, before)
    # NULL q_range: the bytes of pg_quotient (and not those above)
    plain = dict(polys, q_range=None)
    want = call(engine, plain, False)
    assert not torch.equal(want, t)
    assert torch.equal(raw_call(engine, m, x, None, False, bool(m % 2)), want.reshape(4 * n, 4))


@pytest.mark.parametrize("m", range(3, 11))
def test_blinded_random_inputs_equal_the_model(engine, m):
    n = 1 << m
    x, polys = random_inputs(n, seed=900 + m, with_pi=not m % 2, blinded=True)
    before = x.clone()
    t = call(engine, polys, True)
    assert t.shape == (4 * n + 8, 4)
    assert np.array_equal(host(t), PM.limbs_of(RM.quotient_blinded(ints_of(polys), ALPHA, BETA, GAMMA))), m
    assert torch.equal(x, before)
    plain = dict(polys, q_range=None)
    want = call(engine, plain, True)
    assert not torch.equal(want[4 * n:4 * n + 4], t[4 * n:4 * n + 4]) and torch.equal(want[4 * n + 4:], t[4 * n + 4:])
    assert torch.equal(raw_call(engine, m, x, None, True, not m % 2), want)


def polys_c(x, **over):
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


def raw_status(engine, m, p, q_range, blinded, d_t, d_s):
    ks = (pg._lib.Scalar * 4)(*[S(k).c for k in pg.DEFAULT_K])
    return engine._lib.pg_quotient_range(engine._h, m, C.byref(p), q_range, int(blinded), C.byref(S(ALPHA).c), C.byref(S(BETA).c),
                                         C.byref(S(GAMMA).c), C.byref(pg.domain_generator(m + 2).c), ks, C.byref(S(7).c), d_t, d_s,
                                         engine._stream())


def raw_call(engine, m, x, q_range, blinded, with_pi):
    """pg_quotient_range itself on the columns of random_inputs, sentinels behind d_t and the scratch"""
    n = 1 << m
    rows = 4 * n + (8 if blinded else 0)
    t = torch.full((rows + 1, 4), SENTINEL, dtype=torch.int64, device=DEV)
    scratch = torch.full((8 * n + 1, 4), SENTINEL, dtype=torch.int64, device=DEV)
    p = polys_c(x) if with_pi else polys_c(x, pi=None)
    assert raw_status(engine, m, p, q_range, blinded, t.data_ptr(), scratch.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((t[rows] == SENTINEL).all()) and bool((scratch[8 * n] == SENTINEL).all())
    return t[:rows]


@pytest.mark.parametrize("blinded", [False, True])
@pytest.mark.parametrize("m", [3, 6, 10])
def test_sentinels_survive_and_the_python_layer_is_the_c_call(engine, m, blinded):
    n = 1 << m
    x, polys = random_inputs(n, seed=1000 + m, with_pi=True, blinded=blinded)
    before = x.clone()
    t = raw_call(engine, m, x, x[Q_RANGE].data_ptr(), blinded, True)
    assert torch.equal(x, before)  # q_range's sentinel row among them
    assert torch.equal(t, call(engine, polys, blinded).reshape(-1, 4))


def test_error_cases(engine):
    m = 5
    n = 1 << m
    x, polys = random_inputs(n, seed=7, with_pi=True, blinded=True)
    t = torch.zeros((4 * n + 8, 4), dtype=torch.int64, device=DEV)
    scratch = torch.zeros((8, n, 4), dtype=torch.int64, device=DEV)
    p = polys_c(x)
    assert raw_status(engine, m, p, x[Q_RANGE].data_ptr(), True, t.data_ptr(), scratch.data_ptr()) == 0
    torch.cuda.synchronize()
    ref = t.clone()
    row = 32
    both = torch.zeros((n + 4 * n + 8 + n, 4), dtype=torch.int64, device=DEV)  # q_range | d_t | q_range
    bad = {"q_range's last row over d_t": raw_status(engine, m, p, both.data_ptr() + row, True, both.data_ptr() + n * row, scratch.data_ptr()),
           "q_range over d_t's row 4n + 7": raw_status(engine, m, p, both.data_ptr() + (5 * n + 7) * row, True, both.data_ptr() + n * row,
                                                       scratch.data_ptr()),
           "q_range inside the scratch": raw_status(engine, m, p, scratch.data_ptr() + 7 * n * row, True, t.data_ptr(), scratch.data_ptr()),
           "q_range over d_t, unblinded": raw_status(engine, m, p, t.data_ptr() + 3 * n * row, False, t.data_ptr(), scratch.data_ptr()),
           "misaligned q_range": raw_status(engine, m, p, x[Q_RANGE].data_ptr() + 8, True, t.data_ptr(), scratch.data_ptr()),
           "blinded below 2^3": raw_status(engine, 2, p, x[Q_RANGE].data_ptr(), True, t.data_ptr(), scratch.data_ptr()),
           "NULL polys": engine._lib.pg_quotient_range(engine._h, m, None, x[Q_RANGE].data_ptr(), 1, None, None, None, None, None, None,
                                                       t.data_ptr(), scratch.data_ptr(), engine._stream())}
    assert all(st == 2 for st in bad.values()), bad
    torch.cuda.synchronize()
    assert torch.equal(t, ref)  # nothing was launched
    # touching is fine: q_range right in front of d_t and right behind its 4n + 8 rows
    assert raw_status(engine, m, p, both.data_ptr(), True, both.data_ptr() + n * row, scratch.data_ptr()) == 0
    assert raw_status(engine, m, p, both.data_ptr() + (5 * n + 8) * row, True, both.data_ptr() + n * row, scratch.data_ptr()) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        call(engine, dict(polys, q_range=x[Q_RANGE, :n - 1]), True)
    assert np.array_equal(host(call(engine, polys, True)), PM.limbs_of(RM.quotient_blinded(ints_of(polys), ALPHA, BETA, GAMMA)))
