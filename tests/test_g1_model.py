"""CPU: the Python-integer model of BLS12-381 G1 (tests/g1_model.py) against the curve's published facts: the generator is on
y^2 = x^3 + 4, r G = O for the scalar modulus r, its compressed encoding is the known one, and the group law's corner cases."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_model as M  # noqa: E402

G_COMPRESSED = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")


def test_generator_is_on_the_curve_and_has_order_r():
    assert M.on_curve(M.G)
    assert M.mul(M.R_FR, M.G) is None
    assert M.mul(M.R_FR - 1, M.G) == M.neg(M.G)
    assert M.mul(M.R_FR + 5, M.G) == M.mul(5, M.G)


def test_compressed_known_answers():
    assert M.compressed(M.G) == G_COMPRESSED
    assert M.compressed(None) == bytes([0xC0]) + bytes(47)
    # -G has the other sign bit
    ng = M.compressed(M.neg(M.G))
    assert ng[1:] == G_COMPRESSED[1:] and (ng[0] ^ G_COMPRESSED[0]) == 0x20


def test_group_law_corner_cases():
    rng = random.Random(7)
    for _ in range(8):
        p = M.mul(rng.randrange(1, M.R_FR), M.G)
        assert M.on_curve(p)
        assert M.add(p, M.neg(p)) is None
        assert M.add(p, p) == M.mul(2, p)
        assert M.add(p, None) == p and M.add(None, p) == p
        q = M.mul(rng.randrange(1, M.R_FR), M.G)
        assert M.add(p, q) == M.add(q, p)
        assert M.on_curve(M.add(p, q))


def test_naive_msm_is_linear():
    rng = random.Random(11)
    ks = [rng.randrange(M.R_FR) for _ in range(5)]
    ss = [rng.randrange(M.R_FR) for _ in range(5)]
    pts = [M.mul(k, M.G) for k in ks]
    assert M.msm(ss, pts) == M.mul(sum(s * k for s, k in zip(ss, ks)) % M.R_FR, M.G)


def test_limbs_round_trip():
    for v in (0, 1, M.P - 1, M.GX, M.GY):
        assert M.fq_from_limbs(M.fq_limbs(v)) == v
    assert M.point_from_limbs(M.point_limbs(M.G)) == M.G
    assert M.point_from_limbs(M.point_limbs(None)) is None
