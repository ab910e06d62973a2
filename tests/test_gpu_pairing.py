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


@pytest.mark.parametrize("n_pairs", [1, 2, 3, 4, 5, 6, 7, 8])
def test_pair_counts_with_identity_points(engine, n_pairs):
    rng = random.Random(n_pairs)
    h = pg.G2Affine.generator()
    bs = [rng.randrange(1, 1 << 40) for _ in range(n_pairs)]
    prep = [pg.PreparedG2(engine, h.mul(S(b))) for b in bs]
    rows, want = [], []

    def close(ks, at, off):
        """ks with ks[at] replaced so that sum k_j b_j = -off mod r"""
        ks = list(ks)
        ks[at] = 0
        ks[at] = (-(sum(k * b for k, b in zip(ks, bs)) + off)) * pow(bs[at], -1, R) % R
        return ks

    def add(ks):
        rows.append([g1(k) for k in ks])
        want.append(1 if sum(k * b for k, b in zip(ks, bs)) % R == 0 else 0)

    for trial in range(6):
        ks = [rng.randrange(1, 1 << 40) for _ in range(n_pairs)]
        if trial % 2 and n_pairs > 1:
            ks[rng.randrange(n_pairs - 1)] = 0  # an identity P
        # the last scalar closes the product: sum k_j b_j = 0 mod r (or 1 off, on odd trials >= 3)
        off = 1 if trial >= 3 else 0
        add(close(ks, n_pairs - 1, off) if n_pairs > 1 else [0 if not off else 1])
    assert want[:6] == [1, 1, 1, 0, 0, 0]
    # the identity in the LAST position (the slot before it closes the product), then in position 6 with slot 7 or slot 0
    # closing it: the points of slots 6 and 7 are staged in the second LDS slot, their lines selected last in the chain
    holes = [(n_pairs - 1, n_pairs - 2)] if n_pairs > 1 else []
    if n_pairs > 6:
        holes += [(6, n_pairs - 1 if n_pairs == 8 else 0), (6, 5)]
    for hole, closer in holes:
        for off in (0, 1):
            ks = [rng.randrange(1, 1 << 40) for _ in range(n_pairs)]
            ks[hole] = 0
            ks = close(ks, closer, off)
            ks[hole] = 0  # (n_pairs = 2, off = 0: the closer is the identity too)
            add(ks)
            assert want[-1] == 1 - off and (n_pairs == 2 or ks[closer] != 0)
    add([0] * n_pairs)  # every P the identity: the empty product
    assert want[-1] == 1
    assert pg.pairing_check(engine, points(engine, rows), prep).cpu().tolist() == want
    for p in prep:
        p.close()


@pytest.fixture(scope="module")
def e_gh():
    e = M.pairing(G.G, M.G2)
    assert e != M.F12_ONE
    return e


def g2_of(engine, b):
    """b H by the model: (the model's point, its 68 lines, the library's prepared handle of the same point)"""
    q = M.g2_mul(b, M.G2)
    return q, M.g2_prepare(q), pg.PreparedG2(engine, pg.G2Affine.from_ints(*q))


def model_gt(ks, lines):
    """(prod_j e(k_j G, Q_j))^HARD_C: the model's Miller loop over all pairs and its plain final power"""
    pairs = [(G.mul(k % R, G.G) if k % R else None, ln) for k, ln in zip(ks, lines)]
    return M.f12_pow(M.final_exponentiation_plain(M.miller_loop(pairs)), M.HARD_C)


@pytest.mark.parametrize("n_pairs", [5, 6, 7, 8])
def test_gt_of_five_to_eight_pairs(engine, e_gh, n_pairs):
    """full-size distinct scalars in every slot (one b_j = r - 1): exchanging two slots' points or two slots' lines changes the
    value, so the staging of points 6 and 7 and the select chain's pointers 4 .. 7 are pinned limb for limb"""
    rng = random.Random(800 + n_pairs)
    ks = [rng.randrange(1, R) for _ in range(n_pairs)]
    bs = [rng.randrange(1, R) for _ in range(n_pairs)]
    bs[n_pairs - 2] = R - 1
    assert len(set(ks + bs)) == 2 * n_pairs
    qs = [g2_of(engine, b) for b in bs]
    want = model_gt(ks, [ln for _, ln, _ in qs])
    total = sum(k * b for k, b in zip(ks, bs)) % R
    assert want == M.f12_pow(e_gh, M.HARD_C * total % R) and want != M.F12_ONE
    # and no other assignment of points or lines to slots gives it: all k_i b_j sums differ
    for i in range(n_pairs):
        for j in range(i + 1, n_pairs):
            assert (ks[i] - ks[j]) * (bs[i] - bs[j]) % R != 0
    pts = points(engine, [[g1(k) for k in ks]])
    prep = [p for _, _, p in qs]
    assert gt_of(pg.pairing_gt(engine, pts, prep)) == [want]
    assert pg.pairing_check(engine, pts, prep).cpu().tolist() == [0]
    for p in prep:
        p.close()


def test_one_prepared_handle_in_two_slots(engine, e_gh):
    """e(P1, Q) e(P2, Q) with the SAME handle twice in the array"""
    rng = random.Random(22)
    b, a, c = (rng.randrange(1, R) for _ in range(3))
    _, lines, prep = g2_of(engine, b)
    rows = [[g1(a), g1(-a)], [g1(a), g1(1 - a)], [g1(a), g1(c)], [g1(0), g1(c)]]
    pts = points(engine, rows)
    assert pg.pairing_check(engine, pts, [prep, prep]).cpu().tolist() == [1, 0, 0, 0]
    got = gt_of(pg.pairing_gt(engine, pts, [prep, prep]))
    assert got[0] == M.F12_ONE
    assert got[1] == M.f12_pow(e_gh, M.HARD_C * b % R)
    assert got[2] == model_gt([a, c], [lines, lines]) == M.f12_pow(e_gh, M.HARD_C * (a + c) * b % R)
    assert got[3] == M.f12_pow(e_gh, M.HARD_C * c * b % R)
    prep.close()


@pytest.fixture(scope="module")
def eight_rows(e_gh):
    """eight distinct rows of three pairs over full-size b_j H, three of them with product 1 (one of those with an identity
    point), and their GT values: e(G, H)^(3 sum k_j b_j) by the model's power, rows 0 and 5 also through the model's own
    Miller loop and plain final power.  (scalars, b_j, values)"""
    rng = random.Random(4385)
    bs = [rng.randrange(1, R) for _ in range(3)]
    rows = []
    for i in range(8):
        ks = [rng.randrange(1, R) for _ in range(3)]
        if i == 6:
            ks[1] = 0
        if i in (1, 4, 6):
            ks[2] = (-(ks[0] * bs[0] + ks[1] * bs[1])) * pow(bs[2], -1, R) % R
        rows.append(ks)
    expo = [sum(k * b for k, b in zip(ks, bs)) % R for ks in rows]
    assert len(set(expo)) == 6 and [x == 0 for x in expo] == [i in (1, 4, 6) for i in range(8)]
    want = [M.f12_pow(e_gh, M.HARD_C * x % R) for x in expo]
    lines = [M.g2_prepare(M.g2_mul(b, M.G2)) for b in bs]
    for i in (0, 5):
        assert want[i] == model_gt(rows[i], lines)
    assert [w == M.F12_ONE for w in want] == [x == 0 for x in expo]
    return rows, bs, want


def pairing_groups(n_checks):
    """pg_pairing_check's launch (capi_pairing.inc, pairing.hpp): (workgroups, live checks of the last one)"""
    per = 42  # kPairChecks
    groups = (n_checks + per - 1) // per
    return groups, n_checks - (groups - 1) * per


@pytest.mark.parametrize("n_checks", [43, 85])
def test_gt_across_workgroups(engine, eight_rows, n_checks):
    """GT rows written by the second and third workgroup, the last one with a single live check and 41 spare ones"""
    assert pairing_groups(n_checks) == ({43: 2, 85: 3}[n_checks], 1)
    rows, bs, want = eight_rows
    prep = [g2_of(engine, b)[2] for b in bs]
    eight = points(engine, [[g1(k) for k in ks] for ks in rows])
    pts = eight.repeat((n_checks + 7) // 8, 1, 1)[:n_checks].contiguous()
    got = pg.pairing_gt(engine, pts, prep).cpu()
    assert gt_of(got[:8]) == want and gt_of(got[n_checks - 1:]) == [want[(n_checks - 1) % 8]]
    # every row, limb for limb: the model's values as Montgomery limbs, tiled like the points
    signed = lambda w: w - (1 << 64) if w >> 63 else w
    exp = torch.tensor([[signed(w) for w in M.f12_limbs(v)] for v in want], dtype=torch.int64)
    assert torch.equal(got, exp.repeat((n_checks + 7) // 8, 1)[:n_checks])
    ok = pg.pairing_check(engine, pts, prep).cpu().tolist()
    assert ok == [1 if want[i % 8] == M.F12_ONE else 0 for i in range(n_checks)] and 0 < sum(ok) < n_checks
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
