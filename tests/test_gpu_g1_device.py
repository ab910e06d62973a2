"""GPU: the device forms of the G1 group law (csrc/g1.hpp) and batch normalisation (g1_normalize_kernel, csrc/msm.hpp) against
tests/g1_model.py, through the test-only harness tests/cpp/g1_device_ops.hip.

Group law: g1x_add, g1x_add_affine, g1x_dbl, g1x_dbl_affine, g1x_mul_small, g1x_from_affine and g1a_neg over the corpus of
tests/g1_ops_corpus.py (the same point under two different z, P and -P under two different z, a doubled point against a
freshly lifted one, both forms of the identity on either side, k at its bit edges, a few thousand random pairs per operation)
in three launch shapes: full workgroups, one wave per workgroup, and partial waves.

Normalisation: 1, 2, 3 and 32 points per inversion; 1, per_lane - 1, per_lane, per_lane + 1 and 256 per_lane + 1 points (the
last: a second workgroup whose only batch has one point); identities nowhere, everywhere, first or last in every batch, in a
run in the middle, at every other place, and everywhere but the first or the last place of a batch.  Real points must come out
as the model's twelve limbs, identities as twelve zero limbs, and rows past the last point untouched."""
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
import g1_ops_corpus as K  # noqa: E402

DEV = "cuda:0"
# (blocks, threads per block): full workgroups; one wave per workgroup; partial waves (100 = 64 + 36 lanes, an odd grid)
SHAPES = {"full": (1024, 256), "one_wave": (96, 64), "partial_waves": (37, 100)}
SENTINEL = 0x5A5A5A5A5A5A5A5A
PER_LANE = [1, 2, 3, 32]
MASKS = ["none", "all", "first", "last", "middle_run", "every_other", "only_first_real", "only_last_real"]
THREADS = 256  # kThreads: the lanes of a workgroup of g1_normalize_kernel


@pytest.fixture(scope="module")
def lib():
    import g1_device_build
    so = C.CDLL(g1_device_build.build())
    so.g1_op.restype = so.g1_normalize.restype = C.c_int
    so.g1_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    so.g1_normalize.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
    return so


def to_dev(a):
    return None if a is None else torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32).copy()).to(DEV)


@pytest.fixture(scope="module")
def operands():
    """{op: (a, b, k on the device, the model's results)}"""
    return {op: (to_dev(a), to_dev(b), to_dev(k), want) for op, (a, b, k, want) in K.corpus().items()}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("op", list(K.OPS), ids=K.NAMES)
def test_group_law(lib, operands, op, shape):
    a, b, k, want = operands[op]
    n = len(want)
    assert a.shape[0] == n and (b is None or b.shape[0] == n) and (k is None or k.shape[0] == n)
    out = torch.full((n, 12 if op == K.NEG_AFFINE else 24), SENTINEL, dtype=torch.int64, device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    assert lib.g1_op(op, ptr(a), ptr(b), ptr(k), out.data_ptr(), n, *SHAPES[shape]) == 0
    torch.cuda.synchronize()
    bad = K.bad_rows(op, out.cpu().numpy().view(np.uint64), want)
    assert not bad, (K.NAMES[op], shape, bad)


def is_identity(mask, i, m, per_lane):
    """whether input i of m is an identity under the mask; a batch is per_lane consecutive inputs"""
    at, size = i % per_lane, min(per_lane, m - i // per_lane * per_lane)  # the place in the batch, the batch's size
    if mask == "none":
        return False
    if mask == "all":
        return True
    if mask == "first":
        return at == 0
    if mask == "last":
        return at == size - 1
    if mask == "middle_run":  # inside every batch that has an inside; otherwise the middle third of the input
        return 1 <= at <= per_lane - 2 if per_lane >= 3 else m // 3 <= i <= 2 * m // 3
    if mask == "every_other":
        return i % 2 == 1
    if mask == "only_first_real":
        return at != 0
    return at != size - 1


@pytest.fixture(scope="module")
def catalogue():
    """64 known points: their affine limbs, and 32 * 256 + 1 inputs cycling over them, each under a z of its own"""
    pts = K.points()[0][:64]
    rng = random.Random(0x64)
    m = 32 * THREADS + 1
    lifted = K.rows([K.lift(pts[i % 64], rng.randrange(1, K.P)) for i in range(m)])
    affine = np.array([G.point_limbs(p) for p in pts], dtype=np.uint64)
    return affine, lifted


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("per_lane", PER_LANE)
def test_normalize(lib, catalogue, per_lane, mask):
    affine, lifted = catalogue
    for m in sorted({1, max(per_lane - 1, 1), per_lane, per_lane + 1, THREADS * per_lane + 1}):
        ident = np.array([is_identity(mask, i, m, per_lane) for i in range(m)], dtype=bool)
        src = lifted[:m].copy()
        src[ident & (np.arange(m) % 3 != 0), 12:18] = 0  # an identity is ZZ = 0, beside whatever X, Y and ZZZ hold ...
        src[ident & (np.arange(m) % 3 == 0)] = 0         # ... or all zeros
        want = np.full((m + 5, 12), SENTINEL, dtype=np.uint64)
        want[:m] = affine[np.arange(m) % 64]
        want[:m][ident] = 0
        out = torch.full((m + 5, 12), SENTINEL, dtype=torch.int64, device=DEV)
        assert lib.g1_normalize(to_dev(src).data_ptr(), out.data_ptr(), m, per_lane) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (per_lane, mask, m, bad[:8].tolist(), ident[bad[:8]].tolist())
