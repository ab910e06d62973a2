"""GPU: pg_ntt (csrc/ntt.hpp) through Engine.fft / ifft / coset_fft / coset_ifft against the Python-int model of tests/ntt_model.py,
limb for limb, at every size from 1 to 2^16 points (every number and split of passes); bit-exact round trips on the device up to
2^24; the random-point identity at 2^18 and 2^20; every kind at 2^19, 2^21, 2^22, 2^23 (two strided passes, uneven and even splits)
and fft and coset_ifft at 2^25 (three strided passes) through the random-point identity on the host (tests/cpp/ntt_point_check.c);
the error cases; in place vs copying; the composer's wire, sigma and selector polynomials; and one 2^29 column, forward and inverse, its forward result checked on the host by tests/cpp/ntt_point_check.c."""
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
import ntt_model as M  # noqa: E402
import perm_product_model as PM  # noqa: E402
from test_gpu_perm_product import KINDS as CIRCUITS, build  # noqa: E402

DEV = "cuda:0"
KINDS = list(M.KINDS)


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def dev_of(ints):
    return torch.from_numpy(PM.limbs_of(ints).view(np.int64)).to(DEV)


def random_limbs(shape, seed):
    """uniform field elements as Montgomery limbs (every value < q is a valid Montgomery form)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2**64, size=shape + (4,), dtype=np.uint64)
    x[..., 3] %= np.uint64(0x73EDA753299D7D48)  # below q: the top limb is below q's
    return torch.from_numpy(x.view(np.int64)).to(DEV)


def call(engine, kind, x, **kw):
    return getattr(engine, kind)(x, **kw)


@pytest.mark.parametrize("m", range(0, 17))
def test_every_size_and_kind_equals_the_model(engine, m):
    n = 1 << m
    rng = np.random.default_rng(1000 + m)
    one = int(rng.integers(0, n))
    cols3 = [[int(v) ** 5 % M.Q for v in rng.integers(0, 2**62, size=n)],  # random
             [M.Q - 1] * n,                                                 # all q - 1
             [0] * n]                                                       # a single nonzero
    cols3[2][one] = int(rng.integers(1, 2**62)) ** 4 % M.Q
    single = [int(v) ** 3 % M.Q for v in rng.integers(0, 2**62, size=n)]
    for kind in KINDS:
        # three columns at a stride of n + 5 points, transformed in place in the caller's array
        buf = torch.full((3, n + 5, 4), -1, dtype=torch.int64, device=DEV)
        for j in range(3):
            buf[j, :n] = dev_of(cols3[j])
        view = buf[:, :n]
        out = call(engine, kind, view, inplace=True)
        assert out.data_ptr() == buf.data_ptr()
        for j in range(3):
            assert np.array_equal(host(buf[j, :n]), PM.limbs_of(M.KINDS[kind](cols3[j]))), (kind, j)
        assert bool((buf[:, n:] == -1).all()), "a point beyond n of a column was written"
        # one column, copying
        x = dev_of(single)
        got = call(engine, kind, x)
        assert np.array_equal(host(got), PM.limbs_of(M.KINDS[kind](single))), kind
        assert np.array_equal(host(x), PM.limbs_of(single))  # (the input is left alone)
        # zeros stay zeros
        assert bool((call(engine, kind, torch.zeros((n, 4), dtype=torch.int64, device=DEV)) == 0).all())


@pytest.mark.parametrize("m", [20, 21, 24])
def test_round_trips_are_bit_exact(engine, m):
    x = random_limbs((2, 1 << m), seed=m)
    y = engine.ifft(engine.fft(x))
    assert torch.equal(x, y)
    z = engine.coset_ifft(engine.coset_fft(x))
    assert torch.equal(x, z)
    assert torch.equal(engine.fft(engine.ifft(x[1])), x[1])
    assert torch.equal(engine.coset_ifft(engine.coset_fft(x[0], g=5), g=5), x[0])


@pytest.mark.parametrize("m", [18, 20])
def test_random_point_identity(engine, m):
    x = random_limbs((1 << m,), seed=50 + m)
    e = engine.fft(x)
    c, ev = PM.ints_of(host(x)), PM.ints_of(host(e))
    s = 0x5EED_0005 ** 9 % M.Q
    assert M.point_identity_holds(c, ev, s, M.omega_of(m))
    ev[12345] = (ev[12345] + 1) % M.Q
    assert not M.point_identity_holds(c, ev, s, M.omega_of(m))
    # the coset transform is the plain one of c_i g^i
    g = [pow(7, i, M.Q) for i in range(1 << m)]
    ce = PM.ints_of(host(engine.coset_fft(x)))
    assert M.point_identity_holds([a * b % M.Q for a, b in zip(c, g)], ce, s, M.omega_of(m))


def ntt_passes(m):
    """the strided passes of ntt_enqueue (capi.hip) before its last pass of 2^10 points: the top m - 10 bits in passes of at
    most 7 bits, as even as possible, the larger ones first"""
    tile_bits, strided_bits = 10, 7  # kNttTileBits, kNttStridedBits
    if m <= tile_bits:
        return []
    top = m - tile_bits
    count = (top + strided_bits - 1) // strided_bits
    return [top // count + (1 if p < top % count else 0) for p in range(count)]


SPLITS = {19: [5, 4], 21: [6, 5], 22: [6, 6], 23: [7, 6], 25: [5, 5, 5]}


def test_the_splits_the_sizes_below_reach():
    assert {m: ntt_passes(m) for m in SPLITS} == SPLITS
    # (what the other tests of this file reach: one pass up to 2^17, an even pair at 2^20 and 2^24, three passes from 2^25)
    assert [len(ntt_passes(m)) for m in (10, 11, 17, 18, 24, 25, 29)] == [0, 1, 1, 2, 2, 3, 3]
    assert ntt_passes(20) == [5, 5] and ntt_passes(24) == [7, 7]


def device_random(shape, seed):
    """random_limbs, drawn on the device"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randint(-(2**63), 2**63 - 1, tuple(shape) + (4,), dtype=torch.int64, device=DEV, generator=gen)
    x[..., 3] = (x[..., 3] & (2**63 - 1)) % 0x73EDA753299D7D48
    return x


def need_hbm():
    free, _ = torch.cuda.mem_get_info()
    if free < (8 << 30):
        pytest.skip("less than 8 GiB of HBM free")


@pytest.fixture(scope="module")
def scaled_check(tmp_path_factory):
    return M.build_point_check_scaled(str(tmp_path_factory.mktemp("ntt_point_check")))


# (2^25 is 1 GiB per column and its host check takes seconds: the plain forward and the coset inverse kind only)
SPLIT_CASES = [(m, kind) for m in sorted(SPLITS) for kind in KINDS if m < 25 or kind in ("fft", "coset_ifft")]


@pytest.mark.parametrize("m,kind", SPLIT_CASES, ids=["%d-%s" % c for c in SPLIT_CASES])
def test_uneven_and_three_pass_splits(engine, scaled_check, m, kind):
    """one random column of every kind at the sizes of SPLITS: out = kind(in) holds iff the forward side is the (coset) transform
    of the coefficient side, checked at a random point s on the host; one flipped limb of the output breaks it.  At 2^19 also
    three columns in place at a stride of n + 5 points, the points behind each column untouched."""
    need_hbm()
    assert ntt_passes(m) == SPLITS[m]
    n = 1 << m
    rng = np.random.default_rng(7000 + 4 * m + KINDS.index(kind))
    mont = lambda v: np.array(PM.mont(v), dtype=np.uint64)
    s = mont(int.from_bytes(rng.bytes(40), "little") % M.Q)
    om, g = mont(M.omega_of(m)), mont(M.DEFAULT_G if kind.startswith("coset") else 1)
    inverse = kind.endswith("ifft")

    def holds(src, dst):
        c, e = (dst, src) if inverse else (src, dst)
        return scaled_check(c.ctypes.data, e.ctypes.data, n, s.ctypes.data, om.ctypes.data, g.ctypes.data, M.point_check_threads())

    x = device_random((n,), seed=100 * m + KINDS.index(kind))
    src = host(x)
    dst = host(call(engine, kind, x))
    del x
    assert holds(src, dst) == 1
    where = int(rng.integers(0, n))
    dst[where, int(rng.integers(0, 3))] ^= np.uint64(1) << np.uint64(int(rng.integers(0, 64)))
    assert holds(src, dst) == 0, where
    if m != 19:
        return
    buf = torch.full((3, n + 5, 4), -1, dtype=torch.int64, device=DEV)
    buf[:, :n] = device_random((3, n), seed=1900 + KINDS.index(kind))
    before = [np.ascontiguousarray(host(buf[j, :n])) for j in range(3)]
    assert call(engine, kind, buf[:, :n], inplace=True).data_ptr() == buf.data_ptr()
    assert bool((buf[:, n:] == -1).all()), "a point beyond n of a column was written"
    for j in range(3):
        after = np.ascontiguousarray(host(buf[j, :n]))
        assert holds(before[j], after) == 1, j
        after[(where + j) % n, 0] ^= np.uint64(1)
        assert holds(before[j], after) == 0, j


def test_error_cases(engine):
    lib, n = engine._lib, 1 << 10
    x = torch.zeros((2, n, 4), dtype=torch.int64, device=DEV)
    om, g = pg.domain_generator(10), pg.BlsScalar.from_int(7)

    def raw(ptr=None, cols=1, stride=n, log2_n=10, kind=0, omega=om, gen=g):
        return lib.pg_ntt(engine._h, x.data_ptr() if ptr is None else ptr, cols, stride, log2_n, kind, C.byref(omega.c),
                          None if gen is None else C.byref(gen.c), engine._stream())
    assert raw() == 0 and raw(kind=3) == 0 and raw(cols=2) == 0
    bad = {"omega of order 2^11": raw(omega=pg.domain_generator(11)),
           "omega of order 2^9": raw(omega=pg.domain_generator(9)),
           "omega = 1": raw(omega=pg.BlsScalar.from_int(1)),
           "stride < n": raw(cols=2, stride=n - 1),
           "log2_n > 32": raw(log2_n=33, omega=pg.BlsScalar.from_int(1)),
           "NULL data": raw(ptr=0),
           "misaligned data": raw(ptr=x.data_ptr() + 8),
           "unknown kind": raw(kind=4),
           "no coset generator": raw(kind=2, gen=None),
           "zero coset generator": raw(kind=3, gen=pg.BlsScalar.from_int(0))}
    assert all(st == 2 for st in bad.values()), bad
    assert lib.pg_ntt(engine._h, x.data_ptr(), 1, n, 10, 0, None, None, engine._stream()) == 2  # NULL omega
    assert raw(log2_n=0, omega=pg.BlsScalar.from_int(1)) == 0
    # through the Python layer
    with pytest.raises(pg.PgError):
        engine.fft(x, omega=pg.domain_generator(9))
    with pytest.raises(ValueError):
        engine.fft(x[:, : n - 3], inplace=True)
    with pytest.raises(ValueError):
        engine.fft(x, log2_n=9)
    # and the engine goes on
    y = random_limbs((n,), seed=3)
    assert torch.equal(engine.ifft(engine.fft(y)), y)


def test_inplace_equals_copying_and_padding(engine):
    for m in (5, 12, 17):
        x = random_limbs((3, 1 << m), seed=70 + m)
        for kind in KINDS:
            copied = call(engine, kind, x)
            y = x.clone()
            assert call(engine, kind, y, inplace=True).data_ptr() == y.data_ptr()
            assert torch.equal(copied, y), (m, kind)
    # fewer rows than the domain: zero-padded into a new tensor
    x = random_limbs((1000,), seed=9)
    padded = torch.zeros((1024, 4), dtype=torch.int64, device=DEV)
    padded[:1000] = x
    assert torch.equal(engine.ifft(x), engine.ifft(padded))
    assert torch.equal(engine.coset_fft(x, log2_n=12), engine.coset_fft(torch.cat([padded, torch.zeros_like(padded).repeat(3, 1)])))


@pytest.mark.parametrize("circuit", CIRCUITS)
def test_composer_polynomials_equal_the_model(engine, circuit):
    comp = build(engine, circuit)
    n = comp.circuit_size()
    padded_n = 1 << (n - 1).bit_length()
    wp = comp.wire_polynomials()
    sp = comp.sigma_polynomials()
    sel = comp.selector_polynomials()
    assert wp.shape == sp.shape == (4, padded_n, 4) and set(sel) == set(comp.SELECTORS)
    pad = lambda ints: ints + [0] * (padded_n - len(ints))
    vals = comp.wire_values()
    for j in range(4):
        ev = pad(PM.ints_of(host(vals[j])))
        assert np.array_equal(host(wp[j]), PM.limbs_of(M.ifft(ev))), j
    sev = engine.sigma_evaluations(comp.permutation(padded_n))
    for j in range(4):
        assert np.array_equal(host(sp[j]), PM.limbs_of(M.ifft(PM.ints_of(host(sev[j]))))), j
    cols, full = comp.device_columns(), comp.materialize()
    for name in comp.SELECTORS:
        ev = pad(PM.ints_of(host(getattr(cols, name) if name in pg.Columns.SCALAR_COLS else full[name])))
        assert np.array_equal(host(sel[name]), PM.limbs_of(M.ifft(ev))), name
        # and the forward transform gives the column back
        assert np.array_equal(host(engine.fft(sel[name])), PM.limbs_of(ev)), name
    assert np.array_equal(host(engine.fft(wp[0])), PM.limbs_of(pad(PM.ints_of(host(vals[0])))))
    assert torch.equal(engine.fft(sp), sev)
    comp.close()


def test_full_size_column(engine, tmp_path):
    """one random 2^29 column (16 GiB): the forward transform passes the random-point identity, computed on the host by
    tests/cpp/ntt_point_check.c, and ifft(fft(x)) == x bit for bit; the same for coset_ifft(coset_fft(x))"""
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (40 << 30):
        pytest.skip("not enough free HBM for two 2^29 columns")
    m = 29
    check = M.build_point_check(str(tmp_path))
    x = random_limbs((1 << 29,), seed=29)
    e = engine.fft(x)
    c_h, e_h = host(x), host(e)
    s = np.array(PM.mont(0x5EED_0006 ** 13 % M.Q), dtype=np.uint64)
    om = np.array(PM.mont(M.omega_of(m)), dtype=np.uint64)
    assert check(c_h.ctypes.data, e_h.ctypes.data, 1 << m, s.ctypes.data, om.ctypes.data, M.point_check_threads()) == 1
    del c_h, e_h
    engine.ifft(e, inplace=True)
    assert torch.equal(e, x)
    engine.coset_fft(e, inplace=True)
    assert not torch.equal(e, x)
    engine.coset_ifft(e, inplace=True)
    assert torch.equal(e, x)
    del x, e
    gc.collect()
    torch.cuda.empty_cache()
