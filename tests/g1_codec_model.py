"""Python-integer model of G1 ingestion (csrc/g1_codec.hpp) on top of tests/g1_model.py: the 48-byte encoding decoded, the
membership test as plain r P = O, the endomorphism the device's test rests on, and the corpus of encodings and points the host
and device tests share.  Status values are the header's PG_G1_*."""
import random

import g1_model as G

P, R = G.P, G.R_FR
OK, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP, NOT_REDUCED = range(5)
STATUS_NAMES = ("PG_G1_OK", "PG_G1_BAD_ENCODING", "PG_G1_NOT_ON_CURVE", "PG_G1_NOT_IN_SUBGROUP", "PG_G1_NOT_REDUCED")

U = -0xd201000000010000                      # the curve's parameter: r = u^4 - u^2 + 1
LAMBDA = (-U * U) % R                        # a root of lambda^2 + lambda + 1 mod r (the other is u^2 - 1)
# the cube root of unity in Fq with (BETA x, y) = [LAMBDA] (x, y) on G1 (the other one, BETA^2, goes with u^2 - 1)
BETA = 0x5f19672fdf76ce51ba69c6076a0f77eaddb3a93be6f89688de17d813620a00022e01fffffffefffe
GENERATOR_COMPRESSED = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")


def phi(pt):
    return None if pt is None else (BETA * pt[0] % P, pt[1])


def in_subgroup(pt) -> bool:
    """on the curve and r pt = O (the identity included)"""
    return G.on_curve(pt) and G.mul(R, pt) is None


def decode(data: bytes, check_subgroup: bool = True, member=None):
    """48 bytes -> (point, status); the point is None (the identity) whenever the status is not OK.  `member`: the caller's
    knowledge of the point's membership (points built as multiples of the generator), sparing the r P"""
    assert len(data) == 48
    if not data[0] & 0x80:
        return None, BAD_ENCODING
    if data[0] & 0x40:
        return None, (OK if data[0] == 0xC0 and not any(data[1:]) else BAD_ENCODING)
    x = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:], "big")
    if x >= P:
        return None, BAD_ENCODING
    rhs = (x * x * x + 4) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None, NOT_ON_CURVE
    if bool(data[0] & 0x20) != (y > (P - 1) // 2):
        y = (P - y) % P
    if check_subgroup and not (in_subgroup((x, y)) if member is None else member):
        return None, NOT_IN_SUBGROUP
    return (x, y), OK


def check_limbs(limbs) -> int:
    """the status of 12 raw Montgomery limbs (pg_g1_check)"""
    vals = [sum((int(w) & G.MASK) << (64 * i) for i, w in enumerate(limbs[6 * h:6 * h + 6])) for h in (0, 1)]
    if any(v >= P for v in vals):
        return NOT_REDUCED
    pt = G.point_from_limbs(limbs)
    if pt is None:
        return OK
    if not G.on_curve(pt):
        return NOT_ON_CURVE
    return OK if G.mul(R, pt) is None else NOT_IN_SUBGROUP


def raw_x(x: int, flags: int) -> bytes:
    """the encoding with the 381-bit field `x` (not reduced) and the three flag bits"""
    out = bytearray((x & ((1 << 381) - 1)).to_bytes(48, "big"))
    out[0] |= flags
    return bytes(out)


def curve_point_from_x(rng):
    """a point of the curve from a random x: outside the subgroup with probability 1 - 2^-126"""
    while True:
        x = rng.randrange(P)
        rhs = (x * x * x + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return x, (y if rng.random() < 0.5 else P - y)


def subgroup_walk(count, seed):
    """`count` pseudo-random points of G1: a walk k G, (k + s) G, (k + 2 s) G .. by affine additions"""
    rng = random.Random(seed)
    pt, step = G.mul(rng.randrange(1, R), G.G), G.mul(rng.randrange(1, R), G.G)
    out = []
    for _ in range(count):
        out.append(pt)
        pt = G.add(pt, step)
    return out


def corpus(seed=0x6c):
    """(encodings, limb cases): [bytes] for decoding and [12 raw limbs] for the check, edge cases first"""
    rng = random.Random(seed)
    pts = [G.mul(k, G.G) for k in (1, 2, 3, 5, R - 1, R - 2, rng.randrange(R))]
    enc = [G.compressed(p) for p in pts] + [G.compressed(None)]
    # the other sign of y: the same x, bit 5 flipped
    enc += [bytes([e[0] ^ 0x20]) + e[1:] for e in enc[:4]]
    # x = p - 1 (x^3 + 4 = 3: a residue or not, the model says), x = p, p + 1, the largest 381-bit value
    enc += [raw_x(P - 1, 0x80), raw_x(P - 1, 0xA0), raw_x(P, 0x80), raw_x(P + 1, 0xA0), raw_x((1 << 381) - 1, 0x80)]
    # the compressed bit clear: otherwise valid encodings, the all-zero string, an uncompressed-style identity
    enc += [bytes([enc[0][0] & 0x7F]) + enc[0][1:], bytes(48), bytes([0x40]) + bytes(47), bytes([0x20]) + enc[1][1:]]
    # identity encodings with stray bits
    enc += [bytes([0xE0]) + bytes(47), bytes([0xC1]) + bytes(47), bytes([0xC0]) + bytes(46) + b"\x01", bytes([0xC0, 0x80]) + bytes(46),
            bytes([0xC0]) + enc[0][1:]]
    # x values with no square root of x^3 + 4
    found = 0
    x = 0
    while found < 4:
        x += 1
        if pow(x * x * x + 4, (P - 1) // 2, P) != 1:
            enc.append(raw_x(x, 0x80 | (0x20 if found & 1 else 0)))
            found += 1
    enc.append(raw_x(rng.randrange(P), 0x80))  # (whatever a random x is)
    # the order-3 points (0, +-2): on the curve, outside the subgroup
    enc += [G.compressed((0, 2)), G.compressed((0, P - 2))]
    # curve points from random x
    off = [curve_point_from_x(rng) for _ in range(6)]
    enc += [G.compressed(p) for p in off]

    limbs = [G.point_limbs(p) for p in pts + [None, (0, 2), (0, P - 2)] + off]
    # off the curve: a limb of a good point changed, y = 0, x = 0 with another y
    bad = list(G.point_limbs(pts[1]))
    bad[7] ^= 1
    limbs += [bad, G.point_limbs((pts[0][0], 0)), G.fq_limbs(0) + G.fq_limbs(1), G.fq_limbs(5) + [0] * 6]
    # limbs at or above p: a good point's x + p, y + p, the modulus itself, all ones
    for h in (0, 1):
        l = list(G.point_limbs(pts[2]))
        v = sum(w << (64 * i) for i, w in enumerate(l[6 * h:6 * h + 6])) + P
        assert v < 1 << 384
        l[6 * h:6 * h + 6] = [(v >> (64 * i)) & G.MASK for i in range(6)]
        limbs.append(l)
    limbs += [[(P >> (64 * i)) & G.MASK for i in range(6)] + [0] * 6, [G.MASK] * 12]
    return enc, limbs
