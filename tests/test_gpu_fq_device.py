"""GPU: every device form of the base field (csrc/fq.hpp: add, sub, neg, mul, square, to/from Montgomery form, inversion) against
Python integers, limb for limb, through the test-only harness tests/cpp/fq_device_ops.hip: an edge corpus (0, 1, p - 1, R mod p,
values whose high limbs are all ones) crossed with itself, and 2^20 uniform pairs."""
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
import g1_model as M  # noqa: E402

P, RQ = M.P, M.RQ
RINV = pow(RQ, -1, P)
DEV = "cuda:0"
NEG, SQUARE, TO_MONT, FROM_MONT, INVERT = range(5)
ADD, SUB, MUL = range(3)


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the HIP runtime torch loads is the one the harness binds to)
    import fq_device_build
    so = C.CDLL(fq_device_build.build())
    for f in (so.fq_unary, so.fq_binary):
        f.restype = C.c_int
    so.fq_unary.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
    so.fq_binary.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    return so


def to_dev(vals):
    a = np.array([[(v >> (64 * i)) & M.MASK for i in range(6)] for v in vals], dtype=np.uint64).reshape(-1, 6)
    return torch.from_numpy(a.view(np.int64)).to(DEV)


def from_dev(t):
    a = t.cpu().numpy().view(np.uint64)
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in a.tolist()]


def edge_values():
    base = [0, 1, 2, P - 1, P - 2, RQ % P, (P - 1) // 2, (P + 1) // 2, RQ * RQ % P]
    for k in range(1, 6):
        base.append(((1 << 384) - (1 << (64 * k))) % P)  # the high limbs all ones
    base += [(1 << 381) - 1 - P if (1 << 381) - 1 > P else P - 3, 1 << 380, (1 << 64) - 1, (1 << 192) - 1]
    return [v % P for v in base]


def run_binary(lib, op, xs, ys):
    a, b = to_dev(xs), to_dev(ys)
    out = torch.empty_like(a)
    assert lib.fq_binary(op, a.data_ptr(), b.data_ptr(), out.data_ptr(), len(xs)) == 0
    torch.cuda.synchronize()
    return from_dev(out)


def run_unary(lib, op, xs):
    a = to_dev(xs)
    out = torch.empty_like(a)
    assert lib.fq_unary(op, a.data_ptr(), out.data_ptr(), len(xs)) == 0
    torch.cuda.synchronize()
    return from_dev(out)


def model_binary(op, x, y):
    # operands are Montgomery residues: add / sub act on them directly, mul is x y R^-1
    return (x + y) % P if op == ADD else (x - y) % P if op == SUB else x * y * RINV % P


def pairs():
    e = edge_values()
    xs = [x for x in e for _ in e]
    ys = [y for _ in e for y in e]
    rng = random.Random(0xF9)
    xs += [rng.randrange(P) for _ in range(1 << 20)]
    ys += [rng.randrange(P) for _ in range(1 << 20)]
    return xs, ys


@pytest.fixture(scope="module")
def inputs():
    return pairs()


@pytest.mark.parametrize("op", [ADD, SUB, MUL])
def test_binary_ops(lib, inputs, op):
    xs, ys = inputs
    got = run_binary(lib, op, xs, ys)
    bad = [i for i, (x, y, g) in enumerate(zip(xs, ys, got)) if g != model_binary(op, x, y)]
    assert not bad, (op, bad[:5])


def test_unary_ops(lib, inputs):
    xs = inputs[0][: 1 << 16]
    xs = edge_values() + xs
    assert run_unary(lib, NEG, xs) == [(-x) % P for x in xs]
    assert run_unary(lib, SQUARE, xs) == [x * x * RINV % P for x in xs]
    assert run_unary(lib, TO_MONT, xs) == [x * RQ % P for x in xs]
    assert run_unary(lib, FROM_MONT, xs) == [x * RINV % P for x in xs]
    few = xs[:4096]
    # Montgomery in, Montgomery out: (x R^-1)^-1 R = x^-1 R^2; 0 -> 0
    assert run_unary(lib, INVERT, few) == [pow(x, -1, P) * RQ * RQ % P if x else 0 for x in few]
