"""GPU: pg_g1_decompress, pg_g1_check and pg_g1_compress (csrc/g1_codec.hpp) against tests/g1_codec_model.py, bit for bit.

The corpus of the host test plus 2^16 random points (a walk over multiples of G, members by construction, with 256 cofactor
points whose status the model finds by r P) through every entry point, with and without the membership test; batches cut to
full workgroups, one wave and partial waves; one bad point at indices 0, 63, 64 and n - 1 of otherwise good batches; and the
argument errors, which launch nothing."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_codec_model as M  # noqa: E402
import g1_model as G  # noqa: E402

DEV = "cuda:0"
N_BIG = 1 << 16
N_OFF = 256


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def limbs_tensor(rows):
    return torch.from_numpy(np.array(rows, dtype=np.uint64).view(np.int64)).to(DEV)


def limbs_of(t):
    return t.cpu().numpy().view(np.uint64)


def expected_rows(want):
    return np.array([G.point_limbs(pt) for pt, _ in want], dtype=np.uint64), np.array([st for _, st in want], dtype=np.uint8)


def first_bad_of(status):
    bad = np.nonzero(status)[0]
    return int(bad[0]) if len(bad) else len(status)


@pytest.fixture(scope="module")
def big():
    """(encodings, [(point, status)] with the membership test, the same without): the corpus, then N_BIG random points"""
    rng = random.Random(0xC0DEC)
    enc, _ = M.corpus()
    want = [M.decode(e) for e in enc]
    want_nocheck = [M.decode(e, False) for e in enc]
    walk = M.subgroup_walk(N_BIG - N_OFF, 0xB16)
    off = [M.curve_point_from_x(rng) for _ in range(N_OFF)]
    where = set(rng.sample(range(N_BIG), N_OFF))
    wi, oi = iter(walk), iter(off)
    for i in range(N_BIG):
        if i in where:
            pt = next(oi)
            e = G.compressed(pt)
            want.append(M.decode(e))
            assert want[-1][1] == M.NOT_IN_SUBGROUP
            want_nocheck.append((pt, M.OK))
        else:
            pt = next(wi)
            e = G.compressed(pt)
            got = M.decode(e, member=True)
            assert got == (pt, M.OK)
            want.append(got)
            want_nocheck.append(got)
        enc.append(e)
    return enc, want, want_nocheck


def run_decompress(engine, enc, check):
    data = torch.frombuffer(bytearray(b"".join(enc)), dtype=torch.uint8).to(DEV)
    out = torch.empty((len(enc), 12), dtype=torch.int64, device=DEV)
    status, first_bad = engine._g1_decompress_into(data, check, out)
    torch.cuda.synchronize()
    return limbs_of(out), status.cpu().numpy(), int(first_bad.item())


@pytest.mark.parametrize("check", [True, False], ids=["membership", "curve_only"])
def test_decompress_matches_the_model(engine, big, check):
    enc, want, want_nocheck = big
    rows, status = expected_rows(want if check else want_nocheck)
    got_rows, got_status, got_first = run_decompress(engine, enc, check)
    assert np.array_equal(got_status, status), np.nonzero(got_status != status)[0][:8]
    assert np.array_equal(got_rows, rows), np.nonzero((got_rows != rows).any(axis=1))[0][:8]
    assert got_first == first_bad_of(status)
    assert set(status.tolist()) == ({0, 1, 2, 3} if check else {0, 1, 2})
    # the public method: bytes in, the same out
    pts, st = engine.g1_decompress(b"".join(enc[:100]), check_subgroup=check)
    assert np.array_equal(limbs_of(pts), rows[:100]) and np.array_equal(st.cpu().numpy(), status[:100])


@pytest.mark.parametrize("n", [N_BIG, 64, 37, 1, 3 * 256 + 5, 256, 2 * 256], ids=lambda n: "n%d" % n)
def test_launch_shapes(engine, big, n):
    """full workgroups (2^16, 256, 512), one wave (64), partial waves (37, 1, 773): the random part of the batch, cut"""
    enc, want, _ = big
    skip = len(enc) - N_BIG
    rows, status = expected_rows(want[skip:skip + n])
    got_rows, got_status, got_first = run_decompress(engine, enc[skip:skip + n], True)
    assert np.array_equal(got_status, status) and np.array_equal(got_rows, rows)
    assert got_first == first_bad_of(status)
    # the same points back to bytes, and through the check
    pts = limbs_tensor(rows)
    assert engine.g1_compress(pts).cpu().numpy().tobytes() == b"".join(
        e if st == 0 else G.compressed(None) for e, st in zip(enc[skip:skip + n], status))
    st2, fb2 = engine._g1_check(pts)
    assert not st2.any().item() and int(fb2.item()) == n


def test_one_bad_point_is_named_exactly(engine):
    n = 300
    good = M.subgroup_walk(n, 7)
    enc = [G.compressed(p) for p in good]
    rng = random.Random(5)
    off = M.curve_point_from_x(rng)
    x = 1
    while pow(x * x * x + 4, (M.P - 1) // 2, M.P) == 1:
        x += 1
    bads = {M.BAD_ENCODING: bytes([enc[3][0] & 0x7F]) + enc[3][1:], M.NOT_ON_CURVE: M.raw_x(x, 0x80),
            M.NOT_IN_SUBGROUP: G.compressed(off)}
    off_curve = list(G.point_limbs(good[5]))
    off_curve[2] ^= 4
    not_reduced = G.point_limbs(good[6])[:6] + [G.MASK] * 6
    bad_limbs = {M.NOT_ON_CURVE: off_curve, M.NOT_IN_SUBGROUP: G.point_limbs(off), M.NOT_REDUCED: not_reduced}
    good_rows = np.array([G.point_limbs(p) for p in good], dtype=np.uint64)
    for at in (0, 63, 64, n - 1):
        for st, e in bads.items():
            batch = list(enc)
            batch[at] = e
            rows, status, first = run_decompress(engine, batch, True)
            want_status = np.zeros(n, dtype=np.uint8)
            want_status[at] = st
            assert np.array_equal(status, want_status) and first == at, (at, st, first)
            assert not rows[at].any(), "a bad point must come out as the identity"
            keep = np.arange(n) != at
            assert np.array_equal(rows[keep], good_rows[keep])
        for st, l in bad_limbs.items():
            rows = good_rows.copy()
            rows[at] = np.array(l, dtype=np.uint64)
            status, first = engine._g1_check(torch.from_numpy(rows.view(np.int64)).to(DEV))
            want_status = np.zeros(n, dtype=np.uint8)
            want_status[at] = st
            assert np.array_equal(status.cpu().numpy(), want_status) and int(first.item()) == at, (at, st)
    # two bad points: the first one is named
    batch = list(enc)
    batch[200], batch[77] = bads[M.NOT_ON_CURVE], bads[M.NOT_IN_SUBGROUP]
    _, status, first = run_decompress(engine, batch, True)
    assert first == 77 and status[77] == M.NOT_IN_SUBGROUP and status[200] == M.NOT_ON_CURVE


def test_check_and_compress_match_the_model(engine):
    _, limbs = M.corpus()
    want = [M.check_limbs(l) for l in limbs]
    status, first = engine._g1_check(limbs_tensor(limbs))
    assert status.cpu().tolist() == want and int(first.item()) == first_bad_of(np.array(want))
    assert engine.g1_check(limbs_tensor(limbs)).cpu().tolist() == want
    pts = [None, G.G, G.neg(G.G), (0, 2), (0, M.P - 2)] + M.subgroup_walk(500, 11)
    got = engine.g1_compress(limbs_tensor([G.point_limbs(p) for p in pts]))
    assert got.shape == (len(pts), 48) and got.dtype == torch.uint8
    assert got.cpu().numpy().tobytes() == b"".join(G.compressed(p) for p in pts)
    assert got[1].cpu().numpy().tobytes() == M.GENERATOR_COMPRESSED


def test_argument_errors_launch_nothing(engine):
    L, h = engine._lib, engine._h
    n = 8
    data = torch.zeros((48 * n + 16,), dtype=torch.uint8, device=DEV)
    out = torch.zeros((n + 1, 12), dtype=torch.int64, device=DEV)
    status = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    first = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    s = engine._stream()
    d, o, t, f = data.data_ptr(), out.data_ptr(), status.data_ptr(), first.data_ptr()
    bad_calls = [
        lambda: L.pg_g1_decompress(h, d, 0, 1, o, t, f, s),            # n = 0
        lambda: L.pg_g1_decompress(h, d, (1 << 32) + 1, 1, o, t, f, s),
        lambda: L.pg_g1_decompress(h, None, n, 1, o, t, f, s),
        lambda: L.pg_g1_decompress(h, d, n, 1, None, t, f, s),
        lambda: L.pg_g1_decompress(h, d, n, 1, o, None, f, s),
        lambda: L.pg_g1_decompress(h, d, n, 1, o, t, None, s),
        lambda: L.pg_g1_decompress(h, d + 8, n, 1, o, t, f, s),        # misaligned
        lambda: L.pg_g1_decompress(h, d, n, 1, o + 8, t, f, s),
        lambda: L.pg_g1_decompress(h, d, n, 1, o, t, f + 4, s),
        lambda: L.pg_g1_decompress(h, o, n, 1, o, t, f, s),            # in place
        lambda: L.pg_g1_decompress(None, d, n, 1, o, t, f, s),
        lambda: L.pg_g1_check(h, o, 0, t, f, s),
        lambda: L.pg_g1_check(h, None, n, t, f, s),
        lambda: L.pg_g1_check(h, o + 8, n, t, f, s),
        lambda: L.pg_g1_check(h, o, n, None, f, s),
        lambda: L.pg_g1_check(h, o, n, t, f + 4, s),
        lambda: L.pg_g1_compress(h, o, 0, d, s),
        lambda: L.pg_g1_compress(h, None, n, d, s),
        lambda: L.pg_g1_compress(h, o, n, None, s),
        lambda: L.pg_g1_compress(h, o + 8, n, d, s),
        lambda: L.pg_g1_compress(h, o, n, d + 8, s),
        lambda: L.pg_g1_compress(h, o, n, o, s),
    ]
    for i, call in enumerate(bad_calls):
        assert call() == 2, i  # PG_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [9] * n and first.cpu().tolist() == [-5, -5] and not out.any().item() and not data.any().item()
    with pytest.raises(ValueError):
        engine.g1_decompress(b"\x00" * 47)
    with pytest.raises(ValueError):
        engine.g1_decompress(b"")
    with pytest.raises(ValueError):
        engine.g1_check(torch.zeros((0, 12), dtype=torch.int64, device=DEV))
