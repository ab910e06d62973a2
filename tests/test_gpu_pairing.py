"""GPU: pg_pairing_check and pg_pairing_gt against tests/pairing_model.py.

GT values equal the model's plain pairing raised to HARD_C = 3 (the device's final exponentiation computes the cube), limb for
limb; the check accepts e(aG, bH) e(-abG, H) and rejects it with ab + 1; n_pairs = 1 .. 4 with identity points among the P;
n_checks = 1, 63, 64, 65 and 2^12 with a single bad check at index 0, 63, 64 and last, the output naming exactly that index;
NULL pointers and n_pairs = 0 or above the cap are refused."""
import ctypes as C
import os
import random
import sys

import pytest
import torch

import plonk_gadgets_amd as pg

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_model as G  # noqa: E402
import pairing_model as M  # noqa: E402

R = M.R
S = pg.BlsScalar.from_int


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def g1(k):
    return pg.G1Affine.from_ints(*G.mul(k % R, G.G)) if k % R else pg.G1Affine.identity()


def points(engine, rows):
    flat = [p for row in rows for p in row]
    return pg.g1.points_tensor(flat, engine.device).view(len(rows), len(rows[0]), 12)


def gt_of(t):
    return [M.f12_from_limbs([int(w) & G.MASK for w in row]) for row in t.cpu().tolist()]


def test_gt_values_equal_the_models_cubed(engine):
    h = pg.G2Affine.generator()
    b = 0xB0B
    prep_h, prep_bh = pg.PreparedG2(engine, h), pg.PreparedG2(engine, h.mul(S(b)))
    e_gh = M.pairing(G.G, M.G2)
    assert e_gh != M.F12_ONE
    # one pair: e(aG, H)^3 and e(aG, bH)^3
    got = gt_of(pg.pairing_gt(engine, points(engine, [[g1(1)], [g1(5)], [g1(R - 1)], [g1(0)]]), [prep_h]))
    assert got[0] == M.f12_pow(e_gh, 3)
    assert got[1] == M.f12_pow(e_gh, 15)
    assert got[2] == M.f12_pow(e_gh, 3 * (R - 1))
    assert got[3] == M.F12_ONE
    got = gt_of(pg.pairing_gt(engine, points(engine, [[g1(7)]]), [prep_bh]))
    assert got[0] == M.f12_pow(M.pairing(G.mul(7, G.G), M.g2_mul(b, M.G2)), 3) == M.f12_pow(e_gh, 21 * b)
    # two pairs accumulate into one value: e(2G, H) e(3G, bH)
    got = gt_of(pg.pairing_gt(engine, points(engine, [[g1(2), g1(3)]]), [prep_h, prep_bh]))
    assert got[0] == M.f12_pow(e_gh, 3 * (2 + 3 * b))
    prep_h.close()
    prep_bh.close()


def test_accepts_and_rejects(engine):
    h = pg.G2Affine.generator()
    a, b = 0xA11CE, 0xB0B
    prep = [pg.PreparedG2(engine, h.mul(S(b))), pg.PreparedG2(engine, h)]
    rows = [[g1(a), g1(-a * b)], [g1(a), g1(-(a * b + 1))], [g1(0), g1(0)], [g1(0), g1(1)]]
    assert pg.pairing_check(engine, points(engine, rows), prep).cpu().tolist() == [1, 0, 1, 0]
    for p in prep:
        p.close()


@pytest.mark.parametrize("n_pairs", [1, 2, 3, 4])
def test_pair_counts_with_identity_points(engine, n_pairs):
    rng = random.Random(n_pairs)
    h = pg.G2Affine.generator()
    bs = [rng.randrange(1, 1 << 40) for _ in range(n_pairs)]
    prep = [pg.PreparedG2(engine, h.mul(S(b))) for b in bs]
    rows, want = [], []
    for trial in range(6):
        ks = [rng.randrange(1, 1 << 40) for _ in range(n_pairs)]
        if trial % 2 and n_pairs > 1:
            ks[rng.randrange(n_pairs - 1)] = 0  # an identity P
        # the last scalar closes the product: sum k_j b_j = 0 mod r (or 1 off, on odd trials >= 3)
        partial = sum(k * b for k, b in zip(ks[:-1], bs[:-1]))
        off = 1 if trial >= 3 else 0
        ks[-1] = (-(partial + off)) * pow(bs[-1], -1, R) % R if n_pairs > 1 else (0 if not off else 1)
        rows.append([g1(k) for k in ks])
        want.append(0 if off else 1)
    assert pg.pairing_check(engine, points(engine, rows), prep).cpu().tolist() == want
    for p in prep:
        p.close()


@pytest.mark.parametrize("n_checks", [1, 41, 42, 43, 63, 64, 65, 1 << 12])  # (42 checks share a workgroup)
def test_a_single_bad_check_is_named(engine, n_checks):
    h = pg.G2Affine.generator()
    b = 0x5EED
    prep = [pg.PreparedG2(engine, h.mul(S(b))), pg.PreparedG2(engine, h)]
    rng = random.Random(n_checks)
    # a few distinct scalars, tiled (the model's scalar multiplications are the slow part)
    good = [(g1(a), g1(-a * b)) for a in (rng.randrange(1, R) for _ in range(8))]
    bad_a = rng.randrange(1, R)
    bad = (g1(bad_a), g1(-(bad_a * b + 1)))
    base = points(engine, [list(good[i % 8]) for i in range(n_checks)])
    assert pg.pairing_check(engine, base, prep).cpu().tolist() == [1] * n_checks
    for where in sorted({0, 41, 42, 63, 64, n_checks - 1}):
        if where >= n_checks:
            continue
        pts = base.clone()
        pts[where] = points(engine, [list(bad)])[0]
        got = pg.pairing_check(engine, pts, prep).cpu().tolist()
        assert [i for i, x in enumerate(got) if not x] == [where], (n_checks, where)
    for p in prep:
        p.close()


def test_error_cases(engine):
    h = pg.PreparedG2(engine, pg.G2Affine.generator())
    lib, eh = engine._lib, engine._h
    pts = points(engine, [[g1(1)] * 9])
    ok = torch.zeros(1, dtype=torch.uint8, device=engine.device)
    arr = (C.c_void_p * 9)(*[h._h] * 9)
    INVALID = 2
    assert lib.pg_pairing_check(eh, pts.data_ptr(), arr, 1, 0, ok.data_ptr(), None) == INVALID
    assert lib.pg_pairing_check(eh, pts.data_ptr(), arr, 1, 9, ok.data_ptr(), None) == INVALID
    assert lib.pg_pairing_check(eh, None, arr, 1, 1, ok.data_ptr(), None) == INVALID
    assert lib.pg_pairing_check(eh, pts.data_ptr(), None, 1, 1, ok.data_ptr(), None) == INVALID
    assert lib.pg_pairing_check(eh, pts.data_ptr(), arr, 1, 1, None, None) == INVALID
    assert lib.pg_pairing_check(None, pts.data_ptr(), arr, 1, 1, ok.data_ptr(), None) == INVALID
    assert lib.pg_pairing_gt(eh, pts.data_ptr(), arr, 1, 1, None, None) == INVALID
    nul = (C.c_void_p * 1)(None)
    assert lib.pg_pairing_check(eh, pts.data_ptr(), nul, 1, 1, ok.data_ptr(), None) == INVALID
    assert lib.pg_pairing_check(eh, pts.data_ptr(), arr, 0, 1, ok.data_ptr(), None) == 0  # nothing to do
    # pg_g2_prepare refuses the identity and a point off the twist
    out = C.c_void_p()
    assert lib.pg_g2_prepare(eh, C.byref(pg.G2Affine.identity().c), C.byref(out)) == INVALID
    off = list(pg.G2Affine.generator().limbs)
    off[0] ^= 1
    assert lib.pg_g2_prepare(eh, C.byref(pg.G2Affine(off).c), C.byref(out)) == INVALID
    h.close()
