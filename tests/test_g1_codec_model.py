"""CPU: tests/g1_codec_model.py itself -- the pinned encodings, decode o encode = identity, the endomorphism pair (BETA, LAMBDA)
the device's membership test is built on, and the model's two membership tests against each other."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_codec_model as M  # noqa: E402
import g1_model as G  # noqa: E402

P, R = M.P, M.R


def test_pinned_encodings():
    assert G.compressed(G.G) == M.GENERATOR_COMPRESSED
    assert M.GENERATOR_COMPRESSED.hex().startswith("97f1d3a7") and M.GENERATOR_COMPRESSED.hex().endswith("db22c6bb")
    assert M.decode(M.GENERATOR_COMPRESSED) == (G.G, M.OK)
    assert M.decode(bytes([0xC0]) + bytes(47)) == (None, M.OK)
    assert G.compressed(None) == bytes([0xC0]) + bytes(47)
    for bad in (bytes([0xC0]) + bytes(46) + b"\x01", bytes([0xE0]) + bytes(47), bytes(48), bytes([0x40]) + bytes(47)):
        assert M.decode(bad) == (None, M.BAD_ENCODING)


def test_decode_inverts_encode_on_random_multiples():
    rng = random.Random(3)
    for _ in range(40):
        pt = G.mul(rng.randrange(1, R), G.G)
        assert M.decode(G.compressed(pt)) == (pt, M.OK)
        assert M.decode(G.compressed(G.neg(pt))) == (G.neg(pt), M.OK)
    for pt in M.subgroup_walk(200, 9):
        assert M.decode(G.compressed(pt), member=True) == (pt, M.OK)


def test_the_endomorphism_pair():
    u = M.U
    assert u ** 4 - u ** 2 + 1 == R
    assert (M.LAMBDA * M.LAMBDA + M.LAMBDA + 1) % R == 0 and M.LAMBDA == (-u * u) % R
    assert pow(M.BETA, 3, P) == 1 and M.BETA != 1
    # phi(G) = [lambda] G for the chosen pair, and not for the other cube root
    assert M.phi(G.G) == G.mul(M.LAMBDA, G.G)
    assert (M.BETA * M.BETA % P * G.GX % P, G.GY) == G.mul((u * u - 1) % R, G.G) != M.phi(G.G)
    rng = random.Random(4)
    for _ in range(6):
        pt = G.mul(rng.randrange(1, R), G.G)
        assert M.phi(pt) == G.mul(M.LAMBDA, pt)
    # ... and fails for curve points outside the subgroup: the cofactor points and the points of order 3
    for pt in [M.curve_point_from_x(rng) for _ in range(4)] + [(0, 2), (0, P - 2)]:
        assert G.on_curve(pt) and not M.in_subgroup(pt)
        assert M.phi(pt) != G.mul(-(u * u), pt)
    assert G.mul(3, (0, 2)) is None


def test_corpus_covers_every_status():
    enc, limbs = M.corpus()
    seen = {M.decode(e)[1] for e in enc}
    assert seen == {M.OK, M.BAD_ENCODING, M.NOT_ON_CURVE, M.NOT_IN_SUBGROUP}
    assert {M.check_limbs(l) for l in limbs} == {M.OK, M.NOT_ON_CURVE, M.NOT_IN_SUBGROUP, M.NOT_REDUCED}
    # the sign bit alone picks y: both encodings of an x decode to opposite points
    a, b = M.decode(enc[0])[0], M.decode(enc[8])[0]
    assert a == G.neg(b) and a != b
