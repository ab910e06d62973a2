"""Python-integer model of the BLS12-381 base field Fq and of G1 (y^2 = x^3 + 4): the yardstick the device's commitments
are compared with, limb for limb.  Points are (x, y) integer pairs, None the identity; limbs are Montgomery form with
R = 2^384, six 64-bit words, least significant first."""
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R_FR = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001  # the scalar modulus (fr.hpp's q)
B = 4
GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1
G = (GX, GY)
RQ = 1 << 384
MASK = (1 << 64) - 1


def on_curve(pt) -> bool:
    if pt is None:
        return True
    x, y = pt
    return (y * y - x * x * x - B) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    x1, y1 = p1
    x2, y2 = p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


# Jacobian forms for scalar multiplication (no inversion per step)
def _jdbl(p):
    X, Y, Z = p
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    A, Bq = X * X % P, Y * Y % P
    C = Bq * Bq % P
    D = 2 * ((X + Bq) ** 2 - A - C) % P
    E = 3 * A % P
    X3 = (E * E - 2 * D) % P
    return X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P


def _jadd(p, q):
    if p[2] == 0:
        return q
    if q[2] == 0:
        return p
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    Z1Z1, Z2Z2 = Z1 * Z1 % P, Z2 * Z2 % P
    U1, U2 = X1 * Z2Z2 % P, X2 * Z1Z1 % P
    S1, S2 = Y1 * Z2 * Z2Z2 % P, Y2 * Z1 * Z1Z1 % P
    if U1 == U2:
        return _jdbl(p) if S1 == S2 else (1, 1, 0)
    H, r = (U2 - U1) % P, (S2 - S1) % P
    HH = H * H % P
    HHH = H * HH % P
    V = U1 * HH % P
    X3 = (r * r - HHH - 2 * V) % P
    return X3, (r * (V - X3) - S1 * HHH) % P, Z1 * Z2 * H % P


def _to_affine(j):
    if j[2] == 0:
        return None
    zi = pow(j[2], -1, P)
    return j[0] * zi * zi % P, j[1] * zi * zi * zi % P


def mul(k: int, pt):
    """k pt for any integer k (negative: -|k| pt)"""
    if pt is None or k == 0:
        return None
    if k < 0:
        return mul(-k, neg(pt))
    acc, base = (1, 1, 0), (pt[0], pt[1], 1)
    for bit in bin(k)[2:]:
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd(acc, base)
    return _to_affine(acc)


def msm(scalars, points):
    """naive sum of s_i P_i"""
    acc = (1, 1, 0)
    for s, pt in zip(scalars, points):
        q = mul(s, pt)
        if q is not None:
            acc = _jadd(acc, (q[0], q[1], 1))
    return _to_affine(acc)


def fq_limbs(v: int) -> list:
    m = v * RQ % P
    return [(m >> (64 * i)) & MASK for i in range(6)]


def fq_from_limbs(limbs) -> int:
    m = sum((int(w) & MASK) << (64 * i) for i, w in enumerate(limbs))
    return m * pow(RQ, -1, P) % P


def point_limbs(pt) -> list:
    """the 12 limbs of a pg_g1_affine"""
    return [0] * 12 if pt is None else fq_limbs(pt[0]) + fq_limbs(pt[1])


def point_from_limbs(limbs):
    if all(int(w) & MASK == 0 for w in limbs):
        return None
    return fq_from_limbs(limbs[:6]), fq_from_limbs(limbs[6:])


def compressed(pt) -> bytes:
    """48-byte zcash / dusk-bls12_381 encoding"""
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    out = bytearray(pt[0].to_bytes(48, "big"))
    out[0] |= 0x80
    if pt[1] > (P - 1) // 2:
        out[0] |= 0x20
    return bytes(out)
