"""GPU: every device form of the pairing's field tower (csrc/fq2.hpp, csrc/fq12.hpp) against tests/pairing_model.py, limb for limb,
through the test-only harness tests/cpp/fq12_device_ops.hip: Fq2 add, sub, neg, mul, square, inverse, conjugate, the product by
1 + u, doubling and the product by an Fq element; Fq12 add, sub, neg, the per-coefficient product and square, conjugate, the
Frobenius maps p and p^2, the sparse line product and the single-lane inversion.  Inputs: the edge corpus of
tests/test_pairing_host.py (0, 1, u, p - 1 in each coefficient, elements of norm 1) and 2^16 random elements; three launch
shapes: full workgroups, one wave per workgroup, and partial waves."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpp"))
import g1_model as G  # noqa: E402
import pairing_model as M  # noqa: E402
from test_pairing_host import f2_corpus, f12_corpus  # noqa: E402

P, RQ = M.P, G.RQ
RINV = pow(RQ, -1, P)
DEV = "cuda:0"
N_RANDOM = 1 << 16
F2_ADD, F2_SUB, F2_NEG, F2_MUL, F2_SQUARE, F2_INVERSE, F2_CONJ, F2_MUL_XI, F2_DBL, F2_MUL_FQ = range(10)
F12_ADD, F12_SUB, F12_NEG, F12_MUL, F12_SQUARE, F12_CONJ, F12_FROB, F12_FROB2, F12_SPARSE = range(9)
# (blocks, threads per block): full workgroups; one wave per workgroup; partial waves (100 = 64 + 36 lanes, an odd grid)
SHAPES = {"full": (1024, 256), "one_wave": (96, 64), "partial_waves": (37, 100)}


@pytest.fixture(scope="module")
def lib():
    import fq12_device_build
    so = C.CDLL(fq12_device_build.build())
    so.fq2_op.restype = so.fq12_op.restype = so.fq12_inv.restype = C.c_int
    so.fq2_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    so.fq12_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    so.fq12_inv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    return so


def to_dev(fqs, per_row):
    """canonical Fq integers -> int64[len / per_row, 6 per_row] of Montgomery limbs on the device"""
    raw = b"".join((v * RQ % P).to_bytes(48, "little") for v in fqs)
    a = np.frombuffer(raw, dtype=np.uint64).reshape(-1, 6 * per_row)
    return torch.from_numpy(a.view(np.int64).copy()).to(DEV)


def from_dev(t):
    """-> the canonical Fq integers, flat"""
    raw = t.cpu().numpy().tobytes()
    return [int.from_bytes(raw[i:i + 48], "little") * RINV % P for i in range(0, len(raw), 48)]


def flat2(xs):
    return [c for x in xs for c in x]


def flat12(xs):
    return [c for x in xs for co in x for c in co]


def unflat2(v):
    return [(v[i], v[i + 1]) for i in range(0, len(v), 2)]


def unflat12(v):
    return [[(v[i + 2 * k], v[i + 2 * k + 1]) for k in range(6)] for i in range(0, len(v), 12)]


@pytest.fixture(scope="module")
def f2_inputs():
    rng = random.Random(0xF2)
    e = f2_corpus(rng)
    xs = [x for x in e for _ in e] + [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)]
    ys = [y for _ in e for y in e] + [(rng.randrange(P), rng.randrange(P)) for _ in range(N_RANDOM)]
    return xs, ys, to_dev(flat2(xs), 2), to_dev(flat2(ys), 2)


@pytest.fixture(scope="module")
def f12_inputs():
    rng = random.Random(0xF12)
    e = f12_corpus(rng)
    xs = [x for x in e for _ in e[:8]] + [[(rng.randrange(P), rng.randrange(P)) for _ in range(6)] for _ in range(N_RANDOM)]
    ys = [y for _ in e for y in e[-8:]] + [[(rng.randrange(P), rng.randrange(P)) for _ in range(6)] for _ in range(N_RANDOM)]
    e2 = f2_corpus(rng)
    lines = []
    for i in range(len(xs)):
        if i < 4 * len(e2):
            lines.append((e2[i % len(e2)], e2[(i // 3) % len(e2)], ((0, 1, P - 1, rng.randrange(P))[i % 4], 0)))
        else:
            lines.append(((rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), 0)))
    return xs, ys, lines, to_dev(flat12(xs), 12), to_dev(flat12(ys), 12), to_dev([c for ln in lines for f in ln for c in f], 6)


F2_MODEL = {
    F2_ADD: M.f2_add, F2_SUB: M.f2_sub, F2_NEG: lambda a, b: M.f2_neg(a), F2_MUL: M.f2_mul, F2_SQUARE: lambda a, b: M.f2_sqr(a),
    F2_INVERSE: lambda a, b: M.f2_inv(a), F2_CONJ: lambda a, b: M.f2_conj(a), F2_MUL_XI: lambda a, b: M.f2_mul_xi(a),
    F2_DBL: lambda a, b: M.f2_add(a, a), F2_MUL_FQ: lambda a, b: M.f2_scale(a, b[0])}
F12_MODEL = {
    F12_ADD: M.f12_add, F12_SUB: M.f12_sub, F12_NEG: lambda a, b: M.f12_neg(a), F12_MUL: M.f12_mul, F12_SQUARE: lambda a, b: M.f12_sqr(a),
    F12_CONJ: lambda a, b: M.f12_conj(a), F12_FROB: lambda a, b: M.f12_frobenius(a, 1), F12_FROB2: lambda a, b: M.f12_frobenius(a, 2)}
_expected = {}


def expected(key, make):
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def first_bad(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("op", list(F2_MODEL))
def test_fq2_ops(lib, f2_inputs, op, shape):
    xs, ys, dx, dy = f2_inputs
    out = torch.empty_like(dx)
    assert lib.fq2_op(op, dx.data_ptr(), dy.data_ptr(), out.data_ptr(), len(xs), *SHAPES[shape]) == 0
    torch.cuda.synchronize()
    want = expected(("f2", op), lambda: [F2_MODEL[op](a, b) for a, b in zip(xs, ys)])
    got = unflat2(from_dev(out))
    assert len(got) == len(want) and not first_bad(got, want), (op, shape, first_bad(got, want))


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("op", list(F12_MODEL) + [F12_SPARSE])
def test_fq12_coefficient_ops(lib, f12_inputs, op, shape):
    xs, ys, lines, dx, dy, dl = f12_inputs
    out = torch.empty_like(dx)
    assert lib.fq12_op(op, dx.data_ptr(), dy.data_ptr(), dl.data_ptr(), out.data_ptr(), len(xs), *SHAPES[shape]) == 0
    torch.cuda.synchronize()
    if op == F12_SPARSE:
        want = expected(("f12", op), lambda: [M.f12_mul_sparse(a, l0, l2, l3[0]) for a, (l0, l2, l3) in zip(xs, lines)])
    else:
        want = expected(("f12", op), lambda: [F12_MODEL[op](a, b) for a, b in zip(xs, ys)])
    got = unflat12(from_dev(out))
    assert len(got) == len(want) and not first_bad(got, want), (op, shape, first_bad(got, want))


def test_the_frobenius_model_is_the_power_map(f12_inputs):
    """the yardstick of F12_FROB / F12_FROB2 itself: coefficient-wise maps equal x -> x^p and x -> x^(p^2)"""
    for a in f12_inputs[0][-3:]:
        assert M.f12_frobenius(a, 1) == M.f12_pow(a, P) and M.f12_frobenius(a, 2) == M.f12_pow(a, P * P)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fq12_inverse(lib, f12_inputs, shape):
    xs, _, _, dx, _, _ = f12_inputs
    out = torch.empty_like(dx)
    tmp = torch.empty((len(xs), 12 * 12), dtype=torch.int64, device=DEV)
    assert lib.fq12_inv(dx.data_ptr(), out.data_ptr(), tmp.data_ptr(), len(xs), *SHAPES[shape]) == 0
    torch.cuda.synchronize()
    want = expected(("f12", "inv"), lambda: [M.f12_inv(a) for a in xs])
    got = unflat12(from_dev(out))
    assert len(got) == len(want) and not first_bad(got, want), (shape, first_bad(got, want))
    # and in place: out may be the input
    again = dx.clone()
    assert lib.fq12_inv(again.data_ptr(), again.data_ptr(), tmp.data_ptr(), len(xs), *SHAPES[shape]) == 0
    torch.cuda.synchronize()
    assert torch.equal(again, out)
