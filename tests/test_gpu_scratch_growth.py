"""GPU: the engine's grow-only scratch across reallocations.  ONE fresh Engine (every buffer empty) runs, family by family, a
small call, one large enough to outgrow the buffer the small call left, and the small call again -- each result against the
models of tests/ (ntt_model, Horner in Python integers, perm_product_model, g1_model), limb for limb.  Then the engine is closed
and a second one on the same device runs a small call: teardown through the buffers' destructors leaves the device usable."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_model as G  # noqa: E402
import ntt_model as N  # noqa: E402
import perm_product_model as PM  # noqa: E402

DEV = "cuda:0"
S = pg.BlsScalar.from_int
R = G.R_FR
X = 0x5EED_0051 ** 7 % PM.Q
BETA, GAMMA = 0x5EED_0052 ** 9 % PM.Q, 0x5EED_0053 ** 11 % PM.Q
NB = 300  # bases of the MSMs


@pytest.fixture(scope="module")
def engine():
    """not the other files' engine: this one's buffers must start empty"""
    e = pg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def basis():
    """NB small multiples k_i of G with their k_i, and the points as a device tensor (read-only, shared)"""
    rng = random.Random(0x6A0)
    ks = [rng.randrange(1, 2**32) for _ in range(NB)]
    pts = [G.mul(k, G.G) for k in ks]
    return ks, pg.g1.points_tensor([pg.G1Affine(G.point_limbs(p)) for p in pts], DEV)


def host(t):
    return t.cpu().numpy().view(np.uint64)


def dev_ints(ints):
    return torch.from_numpy(PM.limbs_of(ints).view(np.int64)).to(DEV)


def field_ints(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(PM.Q) for _ in range(n)]


def scalars(cols):
    return torch.from_numpy(np.stack([synth.scalars_from_ints(c) for c in cols]).view(np.int64)).to(DEV)


def expect_point(ss, ks):
    return G.point_limbs(G.mul(sum(s * k for s, k in zip(ss, ks)) % R, G.G))


def test_ntt_tables_regrow(engine):
    # 2^11 points cross the 2^10 tile: the tables change shape (lo | hi with H = 2) as well as size; a coset transform keeps two
    for m in (4, 11, 4):
        c = field_ints(1 << m, seed=m)
        assert np.array_equal(host(engine.coset_fft(dev_ints(c))), PM.limbs_of(N.coset_fft(c))), m


def test_poly_evaluate_regrows(engine):
    for n, cols in ((300, 1), (2**14 + 5, 3), (300, 1)):  # 2^14 + 5 coefficients: two segments
        c = [field_ints(n, seed=10 * n + j) for j in range(cols)]
        got = engine.evaluate(torch.stack([dev_ints(x) for x in c]), X)
        assert [v.to_int() for v in got] == [N.horner(x, X) for x in c], (n, cols)


def test_permutation_product_regrows(engine):
    for padded_n in (8, 32768, 8):  # 32768: the smallest power of two above one tile of 16384 rows -- two tiles, two carries
        rng = np.random.default_rng(padded_n)
        sigma = rng.permutation(4 * padded_n).astype(np.int64).reshape(4, padded_n)
        n_values = padded_n - 3
        wires = [field_ints(n_values, seed=padded_n + j) for j in range(4)]
        z, wrap = engine.permutation_product([dev_ints(w) for w in wires], torch.from_numpy(sigma).to(DEV), S(BETA), S(GAMMA))
        ez, ewrap = PM.grand_product(wires, sigma, padded_n, BETA, GAMMA, PM.omega_of(padded_n.bit_length() - 1))
        assert wrap.to_int() == ewrap, padded_n
        assert np.array_equal(host(z), PM.limbs_of(ez)), padded_n


def test_msm_regrows(engine, basis):
    ks, bases = basis
    for n in (1, NB):
        rng = random.Random(n)
        cols = [[rng.randrange(R) for _ in range(n)], [rng.randrange(2**20) for _ in range(n)]]
        got = engine.msm(bases[:n], scalars(cols))
        for j, c in enumerate(cols):
            assert list(got[j].limbs) == expect_point(c, ks[:n]), (n, j)


def test_msm_segmented_regrows(engine, basis):
    ks, bases = basis
    for lengths in ([3], [17, 0, 1, 22], [3]):  # 40 points in four uneven segments, one of them empty
        off = [sum(lengths[:i]) for i in range(len(lengths) + 1)]
        n = off[-1]
        rng = random.Random(n)
        cols = [[rng.randrange(R) for _ in range(n)], [rng.randrange(2**20) for _ in range(n)]][: 1 if n == 3 else 2]
        got = host(engine.msm_segmented(bases[:n], scalars(cols), off)).tolist()
        for s in range(len(lengths)):
            for j, c in enumerate(cols):
                want = expect_point(c[off[s]:off[s + 1]], ks[off[s]:off[s + 1]]) if lengths[s] else [0] * 12
                assert got[s][j] == want, (lengths, s, j)


def test_a_second_engine_after_close(basis):
    ks, bases = basis
    first = pg.Engine(0)
    c = field_ints(16, seed=77)
    assert np.array_equal(host(first.coset_fft(dev_ints(c))), PM.limbs_of(N.coset_fft(c)))
    assert list(first.msm(bases[:1], scalars([[5]]))[0].limbs) == expect_point([5], ks[:1])
    torch.cuda.synchronize()
    first.close()
    second = pg.Engine(0)
    try:
        assert np.array_equal(host(second.coset_fft(dev_ints(c))), PM.limbs_of(N.coset_fft(c)))
        assert [v.to_int() for v in second.evaluate(dev_ints(c), X)] == [N.horner(c, X)]
    finally:
        second.close()
