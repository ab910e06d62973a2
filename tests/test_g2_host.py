"""CPU: the host-only G2 entry points (pg_g2_mul, pg_g2_to_compressed) and G2Affine.from_compressed against
tests/pairing_model.py; the byte round-trips of VerifierKey; the G1 subgroup test of the verifier.  (OpeningKey holds device
memory: its round-trip runs in tests/test_gpu_verify.py.)"""
import ctypes as C
import os
import random
import sys

import pytest

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import _lib
from plonk_gadgets_amd.verifier import g1_in_subgroup

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_model as G  # noqa: E402
import pairing_model as M  # noqa: E402

R, P = M.R, M.P
S = pg.BlsScalar.from_int


def test_mul_and_compressed_match_the_model():
    g = pg.G2Affine.generator()
    assert list(g.limbs) == M.g2_limbs(M.G2)
    rng = random.Random(2)
    for k in [0, 1, 2, 3, R - 1, R - 2, 1 << 200] + [rng.randrange(R) for _ in range(6)]:
        q, want = g.mul(S(k)), M.g2_mul(k, M.G2)
        assert list(q.limbs) == M.g2_limbs(want), hex(k)
        assert q.to_compressed() == M.g2_compressed(want)
        assert pg.G2Affine.from_compressed(q.to_compressed()) == q
        assert q.to_ints() == want
    # k (j G2) = (k j) G2, and NULL means the generator
    out = _lib.G2AffineC()
    assert _lib.load().pg_g2_mul(None, C.byref(S(77).c), C.byref(out)) == 0
    assert pg.G2Affine(list(out.x) + list(out.y)) == g.mul(S(7)).mul(S(11))
    assert g.in_subgroup() and pg.G2Affine.identity().in_subgroup()


def test_mul_refuses_bad_input():
    lib = _lib.load()
    out = _lib.G2AffineC()
    off = list(pg.G2Affine.generator().limbs)
    off[0] ^= 1
    assert lib.pg_g2_mul(C.byref(pg.G2Affine(off).c), C.byref(S(2).c), C.byref(out)) == 2
    assert lib.pg_g2_mul(None, None, C.byref(out)) == 2
    assert lib.pg_g2_mul(C.byref(pg.G2Affine([2**64 - 1] * 24).c), C.byref(S(2).c), C.byref(out)) == 2
    assert lib.pg_g2_to_compressed(C.byref(pg.G2Affine([2**64 - 1] * 24).c), 1, (C.c_uint8 * 96)()) == 2


def twist_point_outside_the_subgroup():
    x0 = 1
    while True:
        x0 += 1
        x = (x0, 1)
        y = M.f2_sqrt(M.f2_add(M.f2_mul(M.f2_sqr(x), x), M.B2))
        if y is not None and M.g2_mul(R, (x, y)) is not None:
            return x, y


def test_from_compressed_rejects_bad_encodings():
    good = pg.G2Affine.generator().mul(S(5)).to_compressed()
    with pytest.raises(ValueError):
        pg.G2Affine.from_compressed(good[:95])
    with pytest.raises(ValueError):
        pg.G2Affine.from_compressed(bytes([good[0] & 0x7F]) + good[1:])          # not flagged compressed
    with pytest.raises(ValueError):
        pg.G2Affine.from_compressed(bytes([0xC0]) + bytes(94) + b"\x01")         # a non-canonical identity
    with pytest.raises(ValueError):                                                # x.c0 = p: not reduced
        pg.G2Affine.from_compressed(bytes([0x80]) + bytes(47) + P.to_bytes(48, "big"))
    assert pg.G2Affine.from_compressed(bytes([0xC0]) + bytes(95)).is_identity()
    # off the twist: walk x.c0 until x^3 + 4 (1 + u) is no square
    x0 = 1
    while M.f2_sqrt(M.f2_add(M.f2_mul(M.f2_sqr((x0, 0)), (x0, 0)), M.B2)) is not None:
        x0 += 1
    with pytest.raises(ValueError, match="twist"):
        pg.G2Affine.from_compressed(bytes([0x80]) + bytes(47) + x0.to_bytes(48, "big"))
    # on the twist, outside the order-r subgroup
    q = twist_point_outside_the_subgroup()
    assert M.on_twist(q)
    with pytest.raises(ValueError, match="subgroup"):
        pg.G2Affine.from_compressed(M.g2_compressed(q))
    assert not pg.G2Affine.from_ints(*q).in_subgroup()
    # the sign bit selects the other root
    flipped = pg.G2Affine.from_compressed(bytes([good[0] ^ 0x20]) + good[1:])
    assert flipped == -pg.G2Affine.from_compressed(good)


def test_g1_subgroup_test():
    assert g1_in_subgroup(pg.G1Affine.identity()) and g1_in_subgroup(pg.G1Affine.generator())
    assert g1_in_subgroup(pg.G1Affine.from_ints(*G.mul(R - 1, G.G)))
    x = 1
    found = 0
    while found < 3:
        x += 1
        rhs = (x ** 3 + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P != rhs:
            continue
        found += 1
        assert g1_in_subgroup(pg.G1Affine.from_ints(x, y)) == (G.mul(R, (x, y)) is None)
        assert not g1_in_subgroup(pg.G1Affine.from_ints(x, y))
    off = list(pg.G1Affine.generator().limbs)
    off[0] ^= 1
    assert not g1_in_subgroup(pg.G1Affine(off))


def test_verifier_key_round_trip():
    names = pg.VerifierKey.NAMES
    assert len(names) == 15
    cms = {k: pg.G1Affine.from_ints(*G.mul(i + 2, G.G)) for i, k in enumerate(names)}
    cms["q_logic"] = pg.G1Affine.identity()
    vk = pg.VerifierKey(1 << 12, cms)
    data = vk.to_bytes()
    assert len(data) == pg.VerifierKey.SIZE == 8 + 15 * 48
    back = pg.VerifierKey.from_bytes(data)
    assert back == vk and back.n == 1 << 12 and back.valid and back.to_bytes() == data
    with pytest.raises(ValueError):
        pg.VerifierKey.from_bytes(data[:-1])
    with pytest.raises(ValueError):
        pg.VerifierKey(12, cms)
    with pytest.raises(ValueError):
        pg.VerifierKey(16, {k: v for k, v in cms.items() if k != "q_m"})
    assert pg.OpeningKey.SIZE == 240
