"""GPU: pg_msm_segmented (csrc/msm_small.hpp) through Engine.msm_segmented against the G1 model (tests/g1_model.py), limb for
limb.  Bases are known multiples k_i G, so a segment's sum is (sum_i s_i k_i mod r) G: one scalar multiplication in the model.
Ragged segments with 1, 2 and 3 columns at a stride; every signed-digit boundary of any window width and the top carry; the
degenerate additions (P + P, P - P, identity bases, zero scalars); agreement with Engine.msm; the launch shapes; more sums than the
normalisation has lanes (2 and 3 sums per inversion, empty segments among them); the argument errors."""
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
NB = 512
INVALID = 2


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def basis():
    """NB random multiples k_i of G with their k_i (read-only, shared), and the same points as a device tensor"""
    rng = random.Random(0x5E6)
    ks = [rng.randrange(1, R) for _ in range(NB)]
    pts = [M.mul(k, M.G) for k in ks]
    return ks, pts, bases_tensor(pts)


def bases_tensor(pts):
    return pg.g1.points_tensor([pg.G1Affine(M.point_limbs(p)) for p in pts], DEV)


def scalars_tensor(cols, stride):
    """columns of canonical ints -> int64[c, n, 4] Montgomery view of a [c, stride, 4] buffer (the tail poisoned)"""
    n = len(cols[0])
    buf = np.full((len(cols), stride, 4), np.uint64(2**64 - 1), dtype=np.uint64)
    for j, c in enumerate(cols):
        buf[j, :n] = synth.scalars_from_ints(c)
    return torch.from_numpy(buf.view(np.int64)).to(DEV)[:, :n]


def offsets_of(lengths):
    off = [0]
    for m in lengths:
        off.append(off[-1] + m)
    return off


def limbs(t):
    """int64[..., 12] on the device -> nested lists of unsigned limbs"""
    return (t.cpu().numpy().view(np.uint64)).tolist()


def expect(scalars, ks):
    return M.point_limbs(M.mul(sum(s * k for s, k in zip(scalars, ks)) % R, M.G))


def check(engine, ks, bases, cols, lengths, stride_extra=5):
    """one call; every (segment, column) against the model"""
    off = offsets_of(lengths)
    n = off[-1]
    assert n == len(ks) == len(cols[0]) == bases.shape[0]
    got = engine.msm_segmented(bases, scalars_tensor(cols, n + stride_extra), off)
    assert got.shape == (len(lengths), len(cols), 12) and got.dtype == torch.int64 and got.device == engine.device
    got = limbs(got)
    for s in range(len(lengths)):
        lo, hi = off[s], off[s + 1]
        for j, c in enumerate(cols):
            assert got[s][j] == expect(c[lo:hi], ks[lo:hi]), (s, j, lo, hi)
    return got


RAGGED = [1, 2, 3, 0, 27, 64, 65, 1, 0, 300]


@pytest.mark.parametrize("n_cols", [1, 2, 3])
def test_ragged_segments(engine, basis, n_cols):
    ks, pts, dev = basis
    n = sum(RAGGED)
    rng = random.Random(100 + n_cols)
    cols = [[rng.randrange(R) for _ in range(n)], [rng.randrange(2**20) for _ in range(n)], [rng.randrange(R) for _ in range(n)]][:n_cols]
    got = check(engine, ks[:n], dev[:n], cols, RAGGED)
    for s, m in enumerate(RAGGED):
        if m == 0:
            assert got[s] == [[0] * 12] * n_cols  # an empty segment: the identity (0, 0)


def edge_scalars():
    out = list(range(18)) + [R - 1, R - 2]
    for k in range(255):
        out += [(2**k - 1) % R, 2**k % R, (2**k + 1) % R]
    return out


@pytest.mark.parametrize("seg_len", [1, 7])
def test_window_edges(engine, basis, seg_len):
    """every signed-digit boundary of every window width, and the top window's carry (r - 1, 2^254 + 1, ...)"""
    ks, pts, dev = basis
    sc = edge_scalars()
    n = len(sc)
    idx = [i % 16 for i in range(n)]
    lengths = [seg_len] * (n // seg_len) + ([n % seg_len] if n % seg_len else [])
    check(engine, [ks[i] for i in idx], dev[idx], [sc], lengths, stride_extra=0)


def test_degenerate_additions(engine, basis):
    ks, pts, dev = basis
    rng = random.Random(7)
    kk, pp, ss, lengths = [], [], [], []
    for reps in (2, 3, 64):  # the same product repeated: P + P occurs in the lanes' sums and in the tree
        s = rng.randrange(R)
        kk += [ks[reps]] * reps
        pp += [pts[reps]] * reps
        ss += [s] * reps
        lengths.append(reps)
    for s in (1, 2, 5, rng.randrange(R)):  # P with s and -P with s: the identity
        kk += [ks[9], R - ks[9]]
        pp += [pts[9], M.neg(pts[9])]
        ss += [s, s]
        lengths.append(2)
    kk += [0, ks[3], 0, 0]  # identity bases, alone and beside a point
    pp += [None, pts[3], None, None]
    ss += [rng.randrange(R), rng.randrange(R), 1, 0]
    lengths += [1, 2, 1]
    kk += ks[:40]  # a segment of zero scalars
    pp += pts[:40]
    ss += [0] * 40
    lengths.append(40)
    small = [rng.randrange(9) for _ in ss]  # small scalars: the accumulator meets +- its own table entries
    got = check(engine, kk, bases_tensor(pp), [ss, small], lengths)
    for s in (3, 4, 5, 6, 7, 9, 10):
        assert got[s][0] == [0] * 12, s


def test_agrees_with_pg_msm(engine, basis):
    ks, pts, dev = basis
    lengths = [1, 63, 64, 65, 1024]
    off = offsets_of(lengths)
    n = off[-1]
    rng = random.Random(11)
    idx = [i % NB for i in range(n)]
    bases = dev[idx]
    sc = scalars_tensor([[rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]], n + 3)
    got = limbs(engine.msm_segmented(bases, sc, torch.tensor(off, dtype=torch.int64)))
    for s in range(len(lengths)):
        lo, hi = off[s], off[s + 1]
        want = engine.msm(bases[lo:hi].contiguous(), sc[:, lo:hi])
        assert [list(p.limbs) for p in want] == got[s], s


@pytest.mark.parametrize("n,n_cols,lengths", [(1, 1, [1]), (63, 1, [63]), (32, 2, [5, 27]), (65, 1, [1, 64]), (257, 1, [256, 1])])
def test_small_launch_shapes(engine, basis, n, n_cols, lengths):
    """n x n_cols of 1, 63, 64, 65 and 257 lanes: below, at and above one wave, and a last wave of one lane"""
    ks, pts, dev = basis
    rng = random.Random(n)
    check(engine, ks[:n], dev[:n], [[rng.randrange(R) for _ in range(n)] for _ in range(n_cols)], lengths)


def test_more_segments_than_resident_waves(engine, basis):
    """4 097 segments of lengths 1, 2, 3, 1, ...: more (segment, column) waves than the sums' grid, which then walks them.  The
    points cycle over 16 (base, scalar) pairs, so a segment's sum is a few model additions of 16 model products"""
    ks, pts, dev = basis
    rng = random.Random(13)
    pair_s = [rng.randrange(R) for _ in range(16)]
    prods = [M.mul(pair_s[i] * ks[i] % R, M.G) for i in range(16)]
    lengths = [1 + s % 3 for s in range(4097)]
    off = offsets_of(lengths)
    n = off[-1]
    idx = [i % 16 for i in range(n)]
    got = limbs(engine.msm_segmented(dev[idx], scalars_tensor([[pair_s[i] for i in idx]], n)[0], off))
    for s in range(4097):
        want = None
        for i in range(off[s], off[s + 1]):
            want = M.add(want, prods[i % 16])
        assert got[s][0] == M.point_limbs(want), s


EMPTY_CYCLE = (0, 1, 2, 1, 0, 0, 3)


def cycled_sums(pair_s, ks, n_segs):
    """the model's sums for segments whose lengths cycle through EMPTY_CYCLE over points cycling through 16 (base, scalar)
    pairs: uint64[n_segs, len(pair_s), 12].  Seven segments take seven points, so the sums repeat every 7 * 16 segments"""
    period = 16 * len(EMPTY_CYCLE)
    rows = np.zeros((period, len(pair_s), 12), dtype=np.uint64)
    for j, col in enumerate(pair_s):
        prods = [M.mul(col[i] * ks[i] % R, M.G) for i in range(16)]
        at = 0
        for s in range(period):
            want = None
            for _ in range(EMPTY_CYCLE[s % 7]):
                want = M.add(want, prods[at % 16])
                at += 1
            rows[s, j] = M.point_limbs(want)
        assert at == period  # (so segment s + period starts at the same place of the points' cycle)
    return np.tile(rows, (n_segs // period + 1, 1, 1))[:n_segs]


@pytest.mark.parametrize("extra,n_cols,per_lane", [(1, 1, 2), (5, 2, 3)])
def test_more_sums_than_normalising_lanes(engine, basis, extra, n_cols, per_lane):
    """num_cus * 256 + 1 sums and 2 (num_cus * 256 + 5): pg_msm_segmented then normalises 2 and 3 sums per inversion, the last
    batch of the first call holding one.  Segment lengths cycle through 0, 1, 2, 1, 0, 0, 3, so empty segments (identities) fall
    first, last and side by side inside the batches"""
    ks, pts, dev = basis
    T = torch.cuda.get_device_properties(0).multi_processor_count * 256
    n_segs = T + extra
    sums = n_segs * n_cols
    assert -(-sums // T) == per_lane and per_lane <= 32, (T, sums)  # (what capi_msm_small.inc computes: not 1 on any device)
    assert sums % per_lane == 1 or extra != 1
    rng = random.Random(17 + extra)
    pair_s = [[rng.randrange(R) for _ in range(16)] for _ in range(n_cols)]
    want = cycled_sums(pair_s, ks, n_segs)
    # the construction itself, against the naive sums of the first 7 * 16 segments
    lengths = [EMPTY_CYCLE[s % 7] for s in range(n_segs)]
    off = offsets_of(lengths)
    n = off[-1]
    for j in range(n_cols):
        for s in range(112):
            idx = [i % 16 for i in range(off[s], off[s + 1])]
            assert want[s, j].tolist() == M.point_limbs(M.msm([pair_s[j][i] for i in idx], [pts[i] for i in idx])), (s, j)
    idx = np.arange(n) % 16
    sc = np.full((n_cols, n + 3, 4), np.uint64(2**64 - 1), dtype=np.uint64)
    for j in range(n_cols):
        sc[j, :n] = synth.scalars_from_ints(pair_s[j])[idx]
    got = engine.msm_segmented(dev[torch.from_numpy(idx).to(DEV)], torch.from_numpy(sc.view(np.int64)).to(DEV)[:, :n], off)
    assert got.shape == (n_segs, n_cols, 12)
    got = got.cpu().numpy().view(np.uint64)
    bad = np.nonzero((got != want).any(axis=2))
    assert bad[0].size == 0, (bad[0][:8].tolist(), bad[1][:8].tolist())
    empty = np.array(lengths) == 0
    assert empty.sum() > n_segs // 3 and not got[empty].any()


def test_one_long_segment_of_srs_powers(engine):
    n = 1 << 14
    ck = pg.CommitKey.setup(engine, n - 1, pg.BlsScalar.from_int(0x5EED_7A0 ** 5))
    sc = torch.from_numpy(synth.uniform_below(2 * n, R, seed=17).view(np.int64)).to(DEV).view(2, n, 4)
    got = limbs(engine.msm_segmented(ck.powers, sc, [0, n]))
    want = engine.msm(ck.powers, sc)
    assert [list(p.limbs) for p in want] == got[0]


def test_argument_errors(engine, basis):
    ks, pts, dev = basis
    lib, h, st = engine._lib, engine._h, engine._stream()
    b = dev[:8].contiguous()
    s = scalars_tensor([[1] * 8, [2] * 8], 8)
    sentinel = 0x5A5A5A5A5A5A5A5A
    out = torch.full((6, 12), sentinel, dtype=torch.int64, device=DEV)
    U = lambda *xs: (C.c_uint64 * len(xs))(*xs)  # noqa: E731
    good = U(0, 3, 8)

    def call(bases=b.data_ptr(), scalars=s.data_ptr(), n=8, n_cols=2, stride=8, off=good, n_segs=2, o=out.data_ptr()):
        return lib.pg_msm_segmented(h, bases, scalars, n, n_cols, stride, off, n_segs, o, st)

    bad = [
        call(off=U(1, 3, 8)), call(off=U(0, 9, 8)), call(off=U(0, 3, 7)), call(off=U(0, 3, 9)), call(off=None),  # a bad table
        call(n=0, off=U(0, 0, 0)),                                  # n = 0 with segments
        call(n_cols=0),
        call(stride=7),
        call(n=1 << 30, n_cols=2, stride=1 << 30, off=U(0, 3, 1 << 30)),  # n x n_cols >= 2^31
        call(n=1 << 31, n_cols=1, stride=1 << 31, off=U(0, 3, 1 << 31)),
        call(n_segs=1 << 30, off=U(0, 8)),                          # n_segs x n_cols >= 2^31 (refused before seg_off is read)
        call(n_segs=1 << 31, n_cols=1, off=U(0, 8)),
        call(bases=None), call(scalars=None), call(o=None),        # NULL
        call(bases=b.data_ptr() + 8), call(scalars=s.data_ptr() + 8), call(o=out.data_ptr() + 8),  # misaligned
        call(o=b.data_ptr() + 96), call(n_segs=1, off=U(0, 8), o=s.data_ptr() + 256),  # d_out overlaps the bases / the scalars
        lib.pg_msm_segmented(None, b.data_ptr(), s.data_ptr(), 8, 2, 8, good, 2, out.data_ptr(), st),
    ]
    torch.cuda.synchronize()
    assert bad == [INVALID] * len(bad), bad
    assert bool((out == sentinel).all()), "a refused call wrote d_out"
    assert bool((b == dev[:8]).all()) and bool((s == scalars_tensor([[1] * 8, [2] * 8], 8)).all())
    assert call(n_segs=0) == 0 and call(n=0, n_segs=0, off=U(0)) == 0  # no segments: nothing to do
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    assert call() == 0
    torch.cuda.synchronize()
    got = limbs(out)
    assert got[0] == expect([1] * 3, ks[:3]) and got[1] == expect([2] * 3, ks[:3])
    assert got[2] == expect([1] * 5, ks[3:8]) and got[3] == expect([2] * 5, ks[3:8])
    assert got[4] == [sentinel] * 12 and got[5] == [sentinel] * 12
    with pytest.raises(ValueError):
        engine.msm_segmented(b, scalars_tensor([[1] * 7], 7)[0], [0, 7])
    with pytest.raises(ValueError):
        engine.msm_segmented(b, s, torch.tensor([0, 8], dtype=torch.int32))
    with pytest.raises(pg.PgError):
        engine.msm_segmented(b, s, [0, 4, 7])
