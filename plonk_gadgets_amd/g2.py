"""BLS12-381 G2 on the host side of verification: G2Affine (the ABI's pg_g2_affine) and OpeningKey (g, h = [1]_2 and [tau]_2,
the last two prepared for pairings on the engine's device).  Scalar multiplication, the encoding and the preparation run in
libplonk_gadgets_hip.so (pg_g2_mul, pg_g2_to_compressed, pg_g2_prepare); decompression is host integers, like G1Affine's."""
from __future__ import annotations

import ctypes as C

from . import _lib
from .g1 import P, G1Affine, _int, _limbs, _MASK
from .transcript import R


def _mul2(a, b):
    return (a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P


def _pow2(a, e):
    out = (1, 0)
    for bit in bin(e)[2:]:
        out = _mul2(out, out)
        if bit == "1":
            out = _mul2(out, a)
    return out


def _sqrt2(a):
    """a square root in Fq2 or None (p = 3 mod 4)"""
    if a == (0, 0):
        return a
    a1 = _pow2(a, (P - 3) // 4)
    alpha, x0 = _mul2(_mul2(a1, a1), a), _mul2(a1, a)
    if alpha == (P - 1, 0):
        cand = _mul2((0, 1), x0)
    else:
        cand = _mul2(_pow2(((1 + alpha[0]) % P, alpha[1]), (P - 1) // 2), x0)
    return cand if _mul2(cand, cand) == a else None


def _check(st, where):
    if st != 0:
        from .engine import PgError
        raise PgError(st, where)


class G2Affine:
    """a point of G2 as the 24 Montgomery limbs of pg_g2_affine (x.c0, x.c1, y.c0, y.c1); all zero is the identity"""
    __slots__ = ("limbs",)

    def __init__(self, limbs):
        limbs = tuple(int(w) & _MASK for w in limbs)
        if len(limbs) != 24:
            raise ValueError("a G2Affine has 24 limbs")
        self.limbs = limbs

    @staticmethod
    def from_ints(x, y) -> "G2Affine":
        return G2Affine(_limbs(x[0] % P) + _limbs(x[1] % P) + _limbs(y[0] % P) + _limbs(y[1] % P))

    @staticmethod
    def identity() -> "G2Affine":
        return G2Affine([0] * 24)

    @staticmethod
    def generator() -> "G2Affine":
        """the library's generator: pg_g2_mul(NULL, 1)"""
        from .scalar import BlsScalar
        out = _lib.G2AffineC()
        _check(_lib.load().pg_g2_mul(None, C.byref(BlsScalar.from_int(1).c), C.byref(out)), "pg_g2_mul")
        return G2Affine(list(out.x) + list(out.y))

    def is_identity(self) -> bool:
        return not any(self.limbs)

    def to_ints(self):
        """((x0, x1), (y0, y1)) as integers, None for the identity"""
        if self.is_identity():
            return None
        v = [_int(self.limbs[6 * i:6 * i + 6]) for i in range(4)]
        return (v[0], v[1]), (v[2], v[3])

    @property
    def c(self) -> "_lib.G2AffineC":
        p = _lib.G2AffineC()
        for i in range(12):
            p.x[i], p.y[i] = self.limbs[i], self.limbs[12 + i]
        return p

    def __neg__(self) -> "G2Affine":
        q = self.to_ints()
        return self if q is None else G2Affine.from_ints(q[0], ((-q[1][0]) % P, (-q[1][1]) % P))

    def mul(self, k) -> "G2Affine":
        """k * self (pg_g2_mul, host)"""
        from .engine import _field
        out = _lib.G2AffineC()
        _check(_lib.load().pg_g2_mul(C.byref(self.c), C.byref(_field(k).c), C.byref(out)), "pg_g2_mul")
        return G2Affine(list(out.x) + list(out.y))

    def in_subgroup(self) -> bool:
        """r * self == O, as (r - 1) * self == -self (the scalars of pg_g2_mul are below r)"""
        return self.is_identity() or self.mul(R - 1) == -self

    def to_compressed(self) -> bytes:
        """the 96-byte zcash / dusk-bls12_381 encoding (pg_g2_to_compressed)"""
        out = (C.c_uint8 * 96)()
        _check(_lib.load().pg_g2_to_compressed(C.byref(self.c), 1, out), "pg_g2_to_compressed")
        return bytes(out)

    @staticmethod
    def from_compressed(data: bytes) -> "G2Affine":
        """the inverse of to_compressed; raises ValueError on an encoding that is not compressed, not canonical, not on the
        twist or -- unlike G1Affine.from_compressed -- not in the order-r subgroup (a key is decoded once)"""
        if len(data) != 96 or not data[0] & 0x80:
            raise ValueError("not a 96-byte compressed G2 encoding")
        if data[0] & 0x40:
            if data[0] != 0xC0 or any(data[1:]):
                raise ValueError("a non-canonical encoding of the identity")
            return G2Affine.identity()
        x1 = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:48], "big")
        x0 = int.from_bytes(data[48:], "big")
        if x0 >= P or x1 >= P:
            raise ValueError("x is not reduced")
        x = (x0, x1)
        x3 = _mul2(_mul2(x, x), x)
        rhs = ((x3[0] + 4) % P, (x3[1] + 4) % P)
        y = _sqrt2(rhs)
        if y is None:
            raise ValueError("not on the twist")
        ny = ((-y[0]) % P, (-y[1]) % P)
        if bool(data[0] & 0x20) != ((y[1], y[0]) > (ny[1], ny[0])):
            y = ny
        q = G2Affine.from_ints(x, y)
        if not q.in_subgroup():
            raise ValueError("not in the order-r subgroup")
        return q

    def __eq__(self, other) -> bool:
        return isinstance(other, G2Affine) and self.limbs == other.limbs

    def __hash__(self) -> int:
        return hash(self.limbs)

    def __repr__(self) -> str:
        return "G2Affine(identity)" if self.is_identity() else "G2Affine(%s)" % self.to_compressed().hex()


class PreparedG2:
    """a pg_g2_prepared: the 68 Miller-loop lines of a G2 point on the engine's device"""

    def __init__(self, engine, point: G2Affine):
        self.engine, self.point = engine, point
        h = C.c_void_p()
        _check(engine._lib.pg_g2_prepare(engine._h, C.byref(point.c), C.byref(h)), "pg_g2_prepare")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.engine._lib.pg_g2_prepared_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OpeningKey:
    """dusk-plonk's OpeningKey: g = [1]_1, h = [1]_2 and tau_h = [tau]_2, the last two prepared on the engine's device"""
    SIZE = 48 + 96 + 96

    def __init__(self, engine, g: G1Affine, h: G2Affine, tau_h: G2Affine):
        if g.is_identity() or h.is_identity() or tau_h.is_identity():
            raise ValueError("an opening key holds no identity")
        # pg_g2_prepare's lines are only meaningful for points of order r: tested here, once per key
        if not (h.in_subgroup() and tau_h.in_subgroup()):
            raise ValueError("h or tau_h is not in the order-r subgroup of the twist")
        self.engine, self.g, self.h, self.tau_h = engine, g, h, tau_h
        self.prepared_h, self.prepared_tau_h = PreparedG2(engine, h), PreparedG2(engine, tau_h)

    @staticmethod
    def setup(engine, tau, base: G1Affine | None = None) -> "OpeningKey":
        """the G2 half of CommitKey.setup's INSECURE development SRS: whoever knows tau can forge proofs"""
        from .engine import _field
        if _field(tau).to_int() == 0:
            raise ValueError("tau = 0")
        h = G2Affine.generator()
        return OpeningKey(engine, base if base is not None else G1Affine.generator(), h, h.mul(tau))

    def to_bytes(self) -> bytes:
        return self.g.to_compressed() + self.h.to_compressed() + self.tau_h.to_compressed()

    @staticmethod
    def from_bytes(engine, data: bytes) -> "OpeningKey":
        """the key of an SRS made elsewhere: no tau needed.  ValueError on a wrong length or a bad point (g must be in G1)"""
        if len(data) != OpeningKey.SIZE:
            raise ValueError(f"an opening key is {OpeningKey.SIZE} bytes, not {len(data)}")
        from .verifier import g1_in_subgroup
        g = G1Affine.from_compressed(data[:48])
        if not g1_in_subgroup(g):
            raise ValueError("g is not in the order-r subgroup")
        return OpeningKey(engine, g, G2Affine.from_compressed(data[48:144]), G2Affine.from_compressed(data[144:]))

    def close(self):
        self.prepared_h.close()
        self.prepared_tau_h.close()
