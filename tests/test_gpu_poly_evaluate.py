"""GPU: pg_poly_evaluate (csrc/quotient.hpp) through Engine.evaluate: Horner in Python integers at every size from 1 to 2^14 that
matters (powers of two, their neighbours, the segment boundaries), several columns at a stride; x = 0 gives c_0; at x = omega^j the
result is fft(c)[j] at 2^20; the error cases; several columns of 259 segments (more partial sums than reduce lanes, more work items
than workgroups) and one 2^28 column, checked by tests/cpp/poly_eval_check.c on the host."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ntt_model as M  # noqa: E402
import perm_product_model as PM  # noqa: E402

DEV = "cuda:0"
X = 0x5EED_0041 ** 11 % PM.Q


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def random_limbs(shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2**64, size=shape + (4,), dtype=np.uint64)
    x[..., 3] %= np.uint64(0x73EDA753299D7D48)
    return torch.from_numpy(x.view(np.int64)).to(DEV)


def ints(t):
    return PM.ints_of(t.cpu().numpy().view(np.uint64))


SIZES = [1, 2, 3, 5, 255, 256, 257, 1000, 1024, 4095, 16383, 16384, 16385, 16384 + 256, 1 << 14 | 1 << 13 | 7]


@pytest.mark.parametrize("n", SIZES)
def test_horner_at_every_size(engine, n):
    # three columns at a stride of n + 3 points, the points beyond n poisoned
    buf = random_limbs((3, n + 3), seed=n)
    buf[:, n:] = -1
    cols = [ints(buf[j, :n]) for j in range(3)]
    got = engine.evaluate(buf[:, :n], X)
    assert [v.to_int() for v in got] == [M.horner(c, X) for c in cols], n
    assert engine.evaluate(buf[1, :n], X)[0].to_int() == M.horner(cols[1], X)
    # x = 0: c_0; x = 1: the sum
    assert [v.to_int() for v in engine.evaluate(buf[:, :n], 0)] == [c[0] for c in cols]
    assert engine.evaluate(buf[2, :n], 1)[0].to_int() == sum(cols[2]) % PM.Q


def test_at_roots_of_unity_it_is_the_fft(engine):
    m = 20
    x = random_limbs((2, 1 << m), seed=20)
    e = engine.fft(x)
    omega = PM.omega_of(m)
    for j in (0, 1, 2, 12345, (1 << m) - 1):
        got = engine.evaluate(x, pow(omega, j, PM.Q))
        assert [v.to_int() for v in got] == [int(PM.ints_of(e[c, j].cpu().numpy().view(np.uint64))[0]) for c in range(2)], j


def test_error_cases(engine):
    lib, n = engine._lib, 1000
    x = random_limbs((2, n), seed=3)
    out = torch.zeros((2, 4), dtype=torch.int64, device=DEV)
    pt = pg.BlsScalar.from_int(X)

    def raw(ptr=None, cols=2, stride=n, size=n, point=pt, dst=None):
        return lib.pg_poly_evaluate(engine._h, x.data_ptr() if ptr is None else ptr, cols, stride, size,
                                    None if point is None else C.byref(point.c), out.data_ptr() if dst is None else dst,
                                    engine._stream())
    assert raw() == 0 and raw(cols=0) == 0
    bad = {"n = 0": raw(size=0), "n > 2^32": raw(size=(1 << 32) + 1, cols=1, stride=(1 << 32) + 1),
           "stride < n": raw(stride=n - 1), "NULL coeffs": raw(ptr=0), "misaligned coeffs": raw(ptr=x.data_ptr() + 8),
           "NULL out": raw(dst=0), "misaligned out": raw(dst=out.data_ptr() + 4), "NULL point": raw(point=None),
           "unreduced point": raw(point=pg.BlsScalar.from_limbs([2**64 - 1] * 4)),
           "overflowing stride": raw(cols=3, stride=1 << 62)}
    assert all(st == 2 for st in bad.values()), bad
    with pytest.raises(ValueError):
        engine.evaluate(x[:, :, :2], X)
    assert [v.to_int() for v in engine.evaluate(x, X)] == [M.horner(ints(x[j]), X) for j in range(2)]


def build_check(out_dir):
    so = os.path.join(out_dir, "libpoly_eval_check.so")
    subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "poly_eval_check.c"), os.path.join(ROOT, "oracle", "fr.c"), "-o", so])
    fn = C.CDLL(so).poly_eval_check
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
    return fn


def eval_launches(n, n_cols, cus):
    """pg_poly_evaluate's launch arithmetic (capi.hip, quotient.hpp): (segments of 16384 points per column, work items
    it = col * segs + seg, workgroups of poly_eval_kernel -- eight per CU, each striding over the items)"""
    seg = 16384  # kEvalSeg
    segs = (n + seg - 1) // seg
    return segs, n_cols * segs, min(n_cols * segs, 8 * cus)


def test_many_segments_in_several_columns(engine, tmp_path):
    """columns of 259 segments: a lane of poly_eval_reduce_kernel sums more than one partial, and x^(16384 seg) comes from a
    table of more than 256 entries; enough columns that poly_eval_kernel's workgroups stride over the items (8 on 256 CUs).
    Every column against Horner on the host, at a random x and at x = 1."""
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (8 << 30):
        pytest.skip("less than 8 GiB of HBM free")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 16384 * 258 + 77
    cols = max(3, 8 * cus // 259 + 1)
    segs, items, grid = eval_launches(n, cols, cus)
    print("poly_evaluate: %d CUs, %d columns of %d points, %d segments each, %d items on %d workgroups"
          % (cus, cols, n, segs, items, grid))
    assert segs == 259 > 256 and items == cols * segs > 8 * cus == grid
    assert eval_launches(n, cols - 1, cus)[1] <= 8 * cus or cols == 3
    check = build_check(str(tmp_path))
    gen = torch.Generator(device=DEV).manual_seed(259)
    buf = torch.randint(-(2**63), 2**63 - 1, (cols, n + 3, 4), dtype=torch.int64, device=DEV, generator=gen)
    buf[..., 3] = (buf[..., 3] & (2**63 - 1)) % 0x73EDA753299D7D48
    buf[:, n:] = -1
    c_h = buf.cpu().numpy().view(np.uint64)
    rng = np.random.default_rng(259)
    out = np.zeros(4, dtype=np.uint64)
    for x in (int.from_bytes(rng.bytes(40), "little") % PM.Q, 1):
        got = engine.evaluate(buf[:, :n], x)
        pt = np.array(PM.mont(x), dtype=np.uint64)
        for j in range(cols):
            assert check(c_h[j].ctypes.data, n, pt.ctypes.data, M.point_check_threads(), out.ctypes.data) == 0
            assert got[j].limbs() == [int(v) for v in out], (x == 1, j)
    assert bool((buf[:, n:] == -1).all())
    assert len({tuple(v.limbs()) for v in got}) == cols  # (the columns differ: a column read for another would show)
    del buf, c_h
    gc.collect()
    torch.cuda.empty_cache()


def test_full_size_column(engine, tmp_path):
    """one random 2^28 column (8 GiB) against Horner on the host"""
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (20 << 30):
        pytest.skip("not enough free HBM for a 2^28 column")
    check = build_check(str(tmp_path))
    x = random_limbs((1 << 28,), seed=28)
    got = engine.evaluate(x, X)[0]
    c_h = x.cpu().numpy().view(np.uint64)
    del x
    pt, out = np.array(PM.mont(X), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    assert check(c_h.ctypes.data, 1 << 28, pt.ctypes.data, M.point_check_threads(), out.ctypes.data) == 0
    assert got.limbs() == [int(v) for v in out]
    gc.collect()
    torch.cuda.empty_cache()
