"""GPU: pg_poly_open and pg_poly_combine (csrc/opening.hpp) through Engine.open / Engine.combine / CommitKey.aggregate_witness.
Limb for limb against tests/opening_model.py at sizes that cross the 2048-point tiles, the lane runs and the carry scan's
levels, with 1 to 32 columns (a column repeated), weights 0, 1 and r - 1, and points 0, 1, r - 1, roots of unity and random
ones; the remainder against Engine.evaluate; the error cases; three columns at the first size whose pass 1 strides over its tiles
(2^22 + 4097 points on 256 CUs), through the division identity at a random point on the host; and 20 columns at n = 2^28
through the division identity at random points and the recurrence at the first, last and tile-edge coefficients.

The model runs on the Montgomery residues themselves: f, q and the remainder are linear in the columns, so with canonical
weights and point the residues obey the same recurrence, and no conversion is needed."""
import ctypes as C
import gc
import os
import random
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import _lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import opening_model as M  # noqa: E402
import perm_product_model as PM  # noqa: E402

DEV = "cuda:0"
R = M.R
RMONT = (1 << 256) % R


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def random_poly(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randint(-(2**63), 2**63 - 1, tuple(shape) + (4,), dtype=torch.int64, device=DEV, generator=g)
    x[..., 3] = (x[..., 3] & (2**63 - 1)) % synth.Q_TOP
    return x


def residues(t):
    """the raw Montgomery residues (x R mod r) of an int64[..., 4] tensor, as ints"""
    a = t.cpu().numpy().view(np.uint64).reshape(-1, 4).tolist()
    return [w0 | w1 << 64 | w2 << 128 | w3 << 192 for w0, w1, w2, w3 in a]


def canonical(res):
    return res * pow(RMONT, -1, R) % R


POINTS = {"zero": 0, "one": 1, "minus_one": R - 1, "omega": pow(PM.omega_of(12), 5, R), "random": 0x5EED_0C0 ** 7 % R}
SIZES = [1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 65537, (1 << 20) + 3]


def columns_for(n, count, seed):
    """`count` columns over at most count - 1 distinct tensors (the last repeats the first) and weights with 0, 1 and r - 1"""
    distinct = max(1, count - 1)
    base = random_poly((distinct, n), seed)
    cols = [base[j] for j in range(distinct)] + ([base[0]] if count > 1 else [])
    rng = random.Random(seed)
    mu = [rng.randrange(R) for _ in range(count)]
    for i, special in enumerate((1, 0, R - 1)):
        if i < count:
            mu[i] = special
    return cols, mu


def model_open(cols, mu, x):
    res = [residues(c) for c in cols]
    return M.ruffini(M.combine(res, mu), x)


@pytest.mark.parametrize("n", SIZES)
def test_limb_for_limb_against_the_model(engine, n):
    counts = (1, 4, 16, 32) if n <= 16385 else (4,)
    for count in counts:
        cols, mu = columns_for(n, count, seed=n * 37 + count)
        for pname in (("random", "minus_one") if n > 4097 else ("random", "zero", "one")):
            x = POINTS[pname]
            w, val = engine.open(cols, mu, x)
            q, rem = model_open(cols, mu, x)
            assert residues(w) == q, (n, count, pname)
            assert canonical(rem) == val.to_int(), (n, count, pname)


@pytest.mark.parametrize("pname", sorted(POINTS))
def test_every_point(engine, pname):
    n, x = 4097 + 2048, POINTS[pname]
    cols, mu = columns_for(n, 6, seed=77)
    w, val = engine.open(cols, mu, x)
    q, rem = model_open(cols, mu, x)
    assert residues(w) == q and canonical(rem) == val.to_int()
    # the remainder is the combination's evaluation
    f = engine.combine(cols, mu)
    assert engine.evaluate(f, x)[0].to_int() == val.to_int()


def test_a_stacked_tensor_and_aggregate_witness(engine):
    n = 3000
    polys = random_poly((5, n), seed=5)
    v, x = 0xABCDEF ** 5 % R, 0x1234 ** 9 % R
    w, val = pg.CommitKey(engine, None).aggregate_witness(polys, x, v)
    q, rem = model_open([polys[j] for j in range(5)], [pow(v, j, R) for j in range(5)], x)
    assert residues(w) == q and canonical(rem) == val.to_int()
    w2, val2 = engine.open([polys[j] for j in range(5)], [pow(v, j, R) for j in range(5)], x)
    assert torch.equal(w, w2) and val == val2


@pytest.mark.parametrize("count", [1, 4, 32])
def test_combine_equals_the_model(engine, count):
    for n in (1, 2049, 70000):
        cols, mu = columns_for(n, count, seed=count + n)
        got = engine.combine(cols, mu)
        assert residues(got) == M.combine([residues(c) for c in cols], mu), (n, count)


def test_error_cases(engine):
    lib, n = engine._lib, 1000
    x = random_poly((3, n), seed=3)
    w = torch.zeros((n + 1, 4), dtype=torch.int64, device=DEV)
    val = torch.zeros((1, 4), dtype=torch.int64, device=DEV)
    pt = pg.BlsScalar.from_int(5)
    bad = _lib.Scalar.of([2**64 - 1] * 4)

    def call(ptrs=None, mu=None, cols=2, size=n, point=pt, wit=None, value=None, raw_point=None):
        ptrs = ptrs if ptrs is not None else [x[0].data_ptr(), x[1].data_ptr()]
        p = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        m = mu if mu is not None else (_lib.Scalar * max(1, len(ptrs)))(*[pg.BlsScalar.from_int(3).c] * len(ptrs))
        return lib.pg_poly_open(engine._h, p, m, cols, size, C.byref(raw_point if raw_point is not None else point.c),
                                w.data_ptr() if wit is None else wit, val.data_ptr() if value is None else value, None)

    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    assert call(size=0) == 2
    assert call(size=(1 << 32) + 1) == 2
    assert call(ptrs=[], cols=0) == 2
    assert call(ptrs=[x[0].data_ptr()] * 33, cols=33) == 2
    assert call(ptrs=[x[0].data_ptr(), 0]) == 2                                 # a NULL column
    assert call(ptrs=[x[0].data_ptr(), x[1].data_ptr() + 8]) == 2               # misaligned
    assert call(wit=0) == 2 and call(value=0) == 2
    assert call(wit=x[1].data_ptr()) == 2                                       # the witness is an input
    assert call(wit=x[0].data_ptr() + 32 * (n - 1)) == 2                        # ... or overlaps one
    assert call(value=x[1].data_ptr() + 32 * 5) == 2                            # the value inside an input
    assert call(value=w.data_ptr() + 32 * 7) == 2                               # the value inside the witness
    assert call(raw_point=bad) == 2                                             # unreduced point
    mu = (_lib.Scalar * 2)(pg.BlsScalar.from_int(1).c, bad)
    assert call(mu=mu) == 2                                                     # unreduced weight
    p = (C.c_void_p * 2)(x[0].data_ptr(), x[1].data_ptr())
    m = (_lib.Scalar * 2)(pg.BlsScalar.from_int(1).c, pg.BlsScalar.from_int(2).c)
    assert lib.pg_poly_combine(engine._h, p, m, 2, n, x[0].data_ptr() + 32, None) == 2   # the output overlaps an input
    assert lib.pg_poly_combine(engine._h, p, m, 0, n, w.data_ptr(), None) == 2
    assert lib.pg_poly_combine(engine._h, p, m, 2, 0, w.data_ptr(), None) == 2
    assert lib.pg_poly_combine(engine._h, None, m, 2, n, w.data_ptr(), None) == 2
    with pytest.raises(ValueError):
        engine.open([x[0], x[1, :10]], [1, 1], 3)
    with pytest.raises(ValueError):
        engine.open([x[0]], [1, 2], 3)
    torch.cuda.synchronize()


def open_launches(n, cus):
    """pg_poly_open's launch arithmetic (capi_open.inc, opening.hpp): (tiles of 2048 points, workgroups of pass 1 -- eight per
    CU, each striding over the tiles --, workgroups of pass 3, tiles per lane of pass 2)"""
    tile = 2048  # kOpenTile
    tiles = (n + tile - 1) // tile
    return tiles, min(tiles, 8 * cus), min(tiles, 2 * cus), (tiles + 255) // 256


def test_pass_one_strides_over_its_tiles(engine, tmp_path):
    """n = 2048 (8 CUs + 2) + 1: three tiles more than pass 1 has workgroups, the last of one point.  With W and val from the
    device and every evaluation by Horner on the host (tests/cpp/poly_eval_check.c): val = sum mu_j p_j(x),
    sum mu_j p_j(r) - val = W(r) (r - x) at a random r, and W[n - 1] = 0 -- W has degree < n - 1, so the random r pins it."""
    from test_gpu_poly_evaluate import build_check
    import ntt_model
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (8 << 30):
        pytest.skip("less than 8 GiB of HBM free")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2048 * (8 * cus + 2) + 1
    tiles, grid1, grid3, chunk = open_launches(n, cus)
    print("poly_open: %d CUs, n = %d, %d tiles, pass 1 on %d workgroups, pass 3 on %d, %d tiles per carry lane"
          % (cus, n, tiles, grid1, grid3, chunk))
    assert tiles == 8 * cus + 3 > grid1 == 8 * cus and open_launches(n - 4097, cus)[0] <= 8 * cus
    check = build_check(str(tmp_path))
    threads = ntt_model.point_check_threads()
    rng = random.Random(n)
    mu = [1, rng.randrange(2, R - 1), R - 1]
    x, r = rng.randrange(R), rng.randrange(R)
    polys = random_poly((3, n), seed=cus)
    w, val = engine.open([polys[j] for j in range(3)], mu, x)
    p_h = polys.cpu().numpy().view(np.uint64)
    w_h = w.cpu().numpy().view(np.uint64)
    del polys, w

    def horner(c, at):
        pt, out = np.array(PM.mont(at), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        assert check(c.ctypes.data, n, pt.ctypes.data, threads, out.ctypes.data) == 0
        return PM.from_mont(out)

    f_x = sum(m * horner(p_h[j], x) for j, m in enumerate(mu)) % R
    f_r = sum(m * horner(p_h[j], r) for j, m in enumerate(mu)) % R
    assert val.to_int() == f_x
    assert not w_h[n - 1].any()
    assert (f_r - f_x) % R == horner(w_h, r) * (r - x) % R
    # one coefficient of W spoiled, in a tile of pass 1's second round: the identity fails
    w_h[2048 * (8 * cus + 1) + 5, 1] ^= np.uint64(1 << 20)
    assert (f_r - f_x) % R != horner(w_h, r) * (r - x) % R
    gc.collect()
    torch.cuda.empty_cache()


def test_full_size_twenty_columns(engine):
    m = 28
    n = 1 << m
    gc.collect()
    torch.cuda.empty_cache()
    base = random_poly((3, n), seed=28)
    rng = random.Random(2028)
    which = [j % 3 for j in range(20)]
    mu = [rng.randrange(R) for _ in range(20)]
    mu[0], mu[1] = 1, R - 1
    x = rng.randrange(R)
    w, val = engine.open([base[j] for j in which], mu, x)
    torch.cuda.synchronize()
    # per distinct tensor, the sum of its weights
    agg = [sum(mu[i] for i in range(20) if which[i] == d) % R for d in range(3)]
    for _ in range(2):
        y = rng.randrange(R)
        ev = [v.to_int() for v in engine.evaluate(base, y)]
        fy = sum(a * e for a, e in zip(agg, ev)) % R
        wy = engine.evaluate(w, y)[0].to_int()
        assert (wy * (y - x) + val.to_int()) % R == fy
    # the recurrence W[i - 1] = f_i + x W[i] (on residues) at the first, last and tile-edge coefficients
    def f_at(i):
        return sum(a * r for a, r in zip(agg, residues(base[:, i]))) % R

    def w_at(i):
        return residues(w[i])[0]

    assert w_at(n - 1) == 0 and w_at(n - 2) == f_at(n - 1)
    assert canonical((f_at(0) + x * w_at(0)) % R) == val.to_int()
    for i in (1, 2, 7, 8, 9, 2047, 2048, 2049, 4096, 1 << 20, (1 << 27) + 2048, n - 2049, n - 2048, n - 2047, n - 3):
        assert w_at(i - 1) == (f_at(i) + x * w_at(i)) % R, i
    del base, w
    gc.collect()
    torch.cuda.empty_cache()
