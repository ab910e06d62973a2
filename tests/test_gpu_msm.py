"""GPU: pg_msm (csrc/msm.hpp) through Engine.msm against the G1 model (tests/g1_model.py), limb for limb.  Bases are known
multiples k_i G, so sum_i s_i P_i = (sum_i s_i k_i mod r) G is one scalar multiplication in the model.  Sizes 1 .. 1024 with
three columns at a stride above n; the digit-boundary scalars of every window; a single hot bucket, repeated bases, P and -P
in one bucket, identity bases and the zero polynomial; and the argument errors."""
import ctypes as C
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
import g1_model as M  # noqa: E402

DEV = "cuda:0"
R = M.R_FR
NMAX = 1024


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def basis():
    """NMAX random multiples k_i of G, with their k_i"""
    rng = random.Random(0xB45E)
    ks = [rng.randrange(1, R) for _ in range(NMAX)]
    return ks, [M.mul(k, M.G) for k in ks]


def bases_tensor(pts):
    return pg.g1.points_tensor([pg.G1Affine(M.point_limbs(p)) for p in pts], DEV)


def scalars_tensor(cols, stride):
    """columns of canonical ints -> int64[c, n, 4] Montgomery view of a [c, stride, 4] buffer (the tail poisoned)"""
    n = len(cols[0])
    buf = np.full((len(cols), stride, 4), np.uint64(2**64 - 1), dtype=np.uint64)
    for j, c in enumerate(cols):
        buf[j, :n] = synth.scalars_from_ints(c)
    return torch.from_numpy(buf.view(np.int64)).to(DEV)[:, :n]


def expect(scalars, ks):
    return M.point_limbs(M.mul(sum(s * k for s, k in zip(scalars, ks)) % R, M.G))


def check(engine, ks, pts, cols, stride_extra=5):
    got = engine.msm(bases_tensor(pts), scalars_tensor(cols, len(cols[0]) + stride_extra))
    for j, c in enumerate(cols):
        assert list(got[j].limbs) == expect(c, ks), j


def special_scalars():
    out = [0, 1, R - 1, R - 2, 2**254, 2**15, 2**16 - 1, 2**16, 2**15 + 1]
    for w in range(16):
        out += [2 ** (16 * w + 15) % R, (2 ** (16 * w + 16) - 1) % R, 2 ** (16 * w + 16) % R, (2 ** (16 * w + 15) + 1) % R]
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 1000, 1024])
def test_sizes_and_columns(engine, basis, n):
    ks, pts = basis
    rng = random.Random(n)
    sp = special_scalars()
    cols = [[rng.randrange(R) for _ in range(n)], [sp[i % len(sp)] for i in range(n)], [rng.randrange(2**20) for _ in range(n)]]
    check(engine, ks[:n], pts[:n], cols)
    # one column alone (int64[n, 4]) gives the same point as its column of the batched call
    one = engine.msm(bases_tensor(pts[:n]), scalars_tensor([cols[0]], n)[0])
    assert list(one[0].limbs) == expect(cols[0], ks[:n])


def test_single_hot_bucket(engine, basis):
    ks, pts = basis
    s = random.Random(3).randrange(R)
    check(engine, ks, pts, [[s] * NMAX, [1] * NMAX, [R - 1] * NMAX])


def test_repeated_bases(engine, basis):
    ks, pts = basis
    rng = random.Random(4)
    n = 777
    idx = [rng.randrange(3) for _ in range(n)]
    check(engine, [ks[i] for i in idx], [pts[i] for i in idx], [[rng.randrange(R) for _ in range(n)], [5] * n])


def test_p_and_minus_p_and_identity_bases(engine, basis):
    ks, pts = basis
    rng = random.Random(6)
    kk, pp, ss = [], [], []
    for i in range(200):
        s = rng.randrange(R)
        kk += [ks[i], R - ks[i], 0]
        pp += [pts[i], M.neg(pts[i]), None]
        ss += [s, s, rng.randrange(R)]
    got = engine.msm(bases_tensor(pp), scalars_tensor([ss], len(ss))[0])
    assert got[0] == pg.G1Affine.identity()
    check(engine, kk, pp, [[rng.randrange(R) for _ in ss], ss])


def test_zero_polynomial_is_the_identity(engine, basis):
    ks, pts = basis
    got = engine.msm(bases_tensor(pts), scalars_tensor([[0] * NMAX, [0] * NMAX], NMAX))
    assert got == [pg.G1Affine.identity()] * 2
    assert got[0].to_compressed() == bytes([0xC0]) + bytes(47)


def test_argument_errors(engine, basis):
    ks, pts = basis
    lib, h = engine._lib, engine._h
    b = bases_tensor(pts[:8])
    s = scalars_tensor([[1] * 8, [2] * 8], 8)
    out = torch.zeros((4, 12), dtype=torch.int64, device=DEV)
    st = engine._stream()
    ok = lib.pg_msm(h, b.data_ptr(), s.data_ptr(), 8, 2, 8, out.data_ptr(), st)
    torch.cuda.synchronize()
    assert ok == 0 and list(pg.g1.points_of(out[:1])[0].limbs) == expect([1] * 8, ks[:8])
    assert lib.pg_msm(h, b.data_ptr(), s.data_ptr(), 0, 1, 8, out.data_ptr(), st) == 2       # n = 0
    assert lib.pg_msm(h, b.data_ptr(), s.data_ptr(), 8, 2, 7, out.data_ptr(), st) == 2       # stride < n
    assert lib.pg_msm(h, None, s.data_ptr(), 8, 1, 8, out.data_ptr(), st) == 2                # NULL
    assert lib.pg_msm(h, b.data_ptr(), None, 8, 1, 8, out.data_ptr(), st) == 2
    assert lib.pg_msm(h, b.data_ptr(), s.data_ptr(), 8, 1, 8, None, st) == 2
    assert lib.pg_msm(h, b.data_ptr() + 8, s.data_ptr(), 8, 1, 8, out.data_ptr(), st) == 2   # misaligned
    assert lib.pg_msm(h, b.data_ptr(), s.data_ptr() + 8, 8, 1, 8, out.data_ptr(), st) == 2
    assert lib.pg_msm(h, b.data_ptr(), s.data_ptr(), 8, 1, 8, out.data_ptr() + 8, st) == 2
    assert lib.pg_msm(h, b.data_ptr(), s.data_ptr(), 8, 1, 8, b.data_ptr() + 96, st) == 2    # d_out overlaps the bases
    assert lib.pg_msm(h, b.data_ptr(), s.data_ptr(), 8, 2, 8, s.data_ptr() + 256, st) == 2   # ... or the scalars
    assert lib.pg_msm(h, b.data_ptr(), s.data_ptr(), 8, 0, 8, out.data_ptr(), st) == 0       # no columns: nothing to do
    with pytest.raises(ValueError):
        engine.msm(b, scalars_tensor([[1] * 7], 7)[0])
