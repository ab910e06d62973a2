"""GPU: pg_msm (csrc/msm.hpp) through Engine.msm against the G1 model (tests/g1_model.py), limb for limb.  Bases are known
multiples k_i G, so sum_i s_i P_i = (sum_i s_i k_i mod r) G is one scalar multiplication in the model.  Sizes 1 .. 1024 with
three columns at a stride above n; the digit-boundary scalars of every window; a single hot bucket, repeated bases, P and -P
in one bucket, identity bases and the zero polynomial; and the argument errors.  At 2^16 + 2^12 points and 37 more, where the
segmented bucket sums take four launches: constant columns, a few distinct values, runs that end on and drift through the lanes'
chunk boundaries, short scalars, and the buckets at the edges of the reduction's segments."""
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


# ---- structured digits beyond two levels of the segmented bucket sums -------------------------------------------------------
# msm_segsum_kernel gives a lane kMsmRun = 64 sorted entries and two output slots, so n entries take the launches counted below.
# N1 = 2^16 + 2^12 goes 1088 -> 34 -> 2 -> 1 lanes: four launches, the partials written to the first pair of buffers, the second,
# the first and the second again, and five workgroups at the first level.  N2 leaves the last lane a chunk of 37.
RUN = 64
N1 = 2**16 + 2**12
N2 = N1 + 37
TOP = 0x73ED  # window 15 of a scalar below r is below this


def segsum_launches(n):
    lanes, launches = -(-n // RUN), [-(-n // RUN)]
    while lanes > 1:
        lanes = -(-2 * lanes // RUN)
        launches.append(lanes)
    return launches


def recode(s):
    """the signed digits of msm.hpp's header comment: window w's raw value (its 16 bits plus the carry of window w - 1) stays
    when it is at most 2^15, else it becomes raw - 2^16 with a carry into window w + 1"""
    digits, carry = [], 0
    for w in range(16):
        raw = ((s >> (16 * w)) & 0xFFFF) + carry
        carry = 1 if raw > 2**15 else 0
        digits.append(raw - 2**16 if carry else raw)
    assert carry == 0 and sum(d << (16 * w) for w, d in enumerate(digits)) == s
    return digits


def from_digits(d):
    """uint16-sized non-negative digits [n, 16] (no window carries) -> the scalars"""
    return [sum(int(v) << (16 * w) for w, v in enumerate(row)) for row in d.tolist()]


def run_digits(n, lengths, rng):
    """[n, 16] digits in [1, 2^15]: in every window the sorted digits form runs whose lengths cycle through `lengths` (the last
    run cut at n), on distinct values of the window's own and in an order of the window's own"""
    counts = []
    while sum(counts) < n:
        counts.append(min(lengths[len(counts) % len(lengths)], n - sum(counts)))
    d = np.empty((n, 16), dtype=np.int64)
    for w in range(16):
        values = np.sort(rng.choice(np.arange(1, (TOP if w == 15 else 2**15 + 1)), size=len(counts), replace=False))
        d[:, w] = rng.permutation(np.repeat(values, counts))
    return d


@pytest.fixture(scope="module")
def wide(basis):
    """N2 bases drawn from the basis by index (indexed on the device), with their multipliers"""
    ks, pts = basis
    idx = np.random.default_rng(0x1D).integers(0, NMAX, size=N2)
    return [ks[i] for i in idx.tolist()], bases_tensor(pts)[torch.from_numpy(idx).to(DEV)]


def check_wide(engine, wide, cols):
    kk, dev = wide
    n = len(cols[0])
    assert all(0 <= s < R for c in cols for s in c)
    got = engine.msm(dev[:n].contiguous(), scalars_tensor(cols, n + 11))
    for j, c in enumerate(cols):
        assert list(got[j].limbs) == expect(c, kk[:n]), j


def test_structured_sizes_take_four_launches():
    assert segsum_launches(N1) == [1088, 34, 2, 1] and segsum_launches(N2) == [1089, 35, 2, 1]
    assert -(-1088 // 256) == 5 and N2 % RUN == 37


@pytest.mark.parametrize("n", [N1, N2])
def test_constant_columns(engine, wide, n):
    """one hot bucket per window: a run open across every lane and through all four levels"""
    s = random.Random(21).randrange(R)
    check_wide(engine, wide, [[s] * n, [1] * n, [R - 1] * n])
    check_wide(engine, wide, [[2**15] * n])


@pytest.mark.parametrize("n", [N1, N2])
def test_few_distinct_values(engine, wide, n):
    rng = random.Random(22)
    a, b = rng.randrange(R), rng.randrange(R)
    four = [rng.randrange(R) for _ in range(4)]
    check_wide(engine, wide, [[(a, b)[i % 2] for i in range(n)], [four[min(4 * i // n, 3)] for i in range(n)]])


def test_runs_on_chunk_boundaries(engine, wide):
    """every window: N1 / 64 digit values, 64 times each, so every sorted run starts and ends where a lane's chunk does"""
    d = run_digits(N1, [RUN], np.random.default_rng(23))
    for w in range(16):
        values, counts = np.unique(d[:, w], return_counts=True)
        assert len(values) == N1 // RUN and (counts == RUN).all() and values[0] >= 1 and values[-1] <= 2**15
    col = from_digits(d)
    assert recode(col[0]) == d[0].tolist() and recode(col[-1]) == d[-1].tolist()
    check_wide(engine, wide, [col])


@pytest.mark.parametrize("n", [N1, N2])
def test_runs_drifting_through_the_chunks(engine, wide, n):
    """runs of 63 and 65 in turn: the runs' ends move through every place of the lanes' chunks"""
    d = run_digits(n, [63, 65], np.random.default_rng(24))
    col = from_digits(d)
    assert recode(col[1]) == d[1].tolist()
    check_wide(engine, wide, [col])


@pytest.mark.parametrize("n", [N1, N2])
def test_short_scalars(engine, wide, n):
    """below 2^20 and below 2^16: windows 2 .. 15 (1 .. 15) are one run of zero digits over every lane and level"""
    rng = random.Random(25)
    check_wide(engine, wide, [[rng.randrange(2**20) for _ in range(n)], [rng.randrange(2**16) for _ in range(n)]])


EDGE_BUCKETS = [1, 127, 128, 129, 255, 256, 257, 2**15 - 129, 2**15 - 128, 2**15 - 127, 2**15 - 1]


def test_bucket_segment_edges(engine, wide):
    """msm_bucket_reduce_kernel sums segments of 128 buckets, [128 j + 1, 128 j + 128], and scales a segment's total by 128 j:
    every window gets points in the buckets at the edges of the first, second, third and last segments, under both signs, and
    in bucket 2^15.  A scalar is built from its signed digits -- the wanted one in window w, small ones elsewhere -- and the
    recoding rule is applied to it to check them.  (Below r the top window holds 0 .. 0x73ed, so it takes the positive edges up
    to 257 only.)"""
    rng = random.Random(26)
    col, seen = [], set()
    for w in range(16):
        for d in EDGE_BUCKETS + [-b for b in EDGE_BUCKETS] + [2**15]:
            if w == 15 and not 0 <= d < TOP:
                continue
            for _ in range(6):
                digits = [rng.randrange(-2, 3) for _ in range(16)]
                digits[15] = rng.randrange(1, 4)
                digits[w] = d
                s = sum(v << (16 * i) for i, v in enumerate(digits))
                assert 0 < s < R and recode(s) == digits
                col.append(s)
            seen.add((w, d))
    assert len(seen) == 15 * 23 + 7 and len(col) >= 2048
    check_wide(engine, wide, [col])


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
