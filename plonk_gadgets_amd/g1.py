"""BLS12-381 G1 on the host side of the commitments: G1Affine (the ABI's pg_g1_affine), CommitKey (the powers tau^i G of an
insecure development SRS, on the device) and PolynomialDegreeTooLarge.  The arithmetic runs in libplonk_gadgets_hip.so
(pg_msm, pg_srs_setup, pg_g1_to_compressed); this module only converts."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
_R = 1 << 384
_MASK = (1 << 64) - 1
_GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
_GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1


class PolynomialDegreeTooLarge(ValueError):
    """a polynomial longer than the commit key (dusk-plonk's Error::PolynomialDegreeTooLarge)"""


def _limbs(v: int) -> list:
    m = v * _R % P
    return [(m >> (64 * i)) & _MASK for i in range(6)]


def _int(limbs) -> int:
    return sum((int(w) & _MASK) << (64 * i) for i, w in enumerate(limbs)) * pow(_R, -1, P) % P


class G1Affine:
    """a point of G1 as the 12 Montgomery limbs of pg_g1_affine (x then y); (0, 0) is the identity"""
    __slots__ = ("limbs",)

    def __init__(self, limbs):
        limbs = tuple(int(w) & _MASK for w in limbs)
        if len(limbs) != 12:
            raise ValueError("a G1Affine has 12 limbs")
        self.limbs = limbs

    @staticmethod
    def from_ints(x: int, y: int) -> "G1Affine":
        return G1Affine(_limbs(x % P) + _limbs(y % P))

    @staticmethod
    def identity() -> "G1Affine":
        return G1Affine([0] * 12)

    @staticmethod
    def generator() -> "G1Affine":
        return G1Affine.from_ints(_GX, _GY)

    def is_identity(self) -> bool:
        return not any(self.limbs)

    def to_ints(self):
        """(x, y) as integers, None for the identity"""
        return None if self.is_identity() else (_int(self.limbs[:6]), _int(self.limbs[6:]))

    @property
    def c(self) -> "_lib.G1AffineC":
        p = _lib.G1AffineC()
        for i in range(6):
            p.x[i], p.y[i] = self.limbs[i], self.limbs[6 + i]
        return p

    def to_compressed(self) -> bytes:
        """the 48-byte zcash / dusk-bls12_381 encoding (pg_g1_to_compressed)"""
        out = (C.c_uint8 * 48)()
        st = _lib.load().pg_g1_to_compressed(C.byref(self.c), 1, out)
        if st != 0:
            from .engine import PgError
            raise PgError(st, "pg_g1_to_compressed")
        return bytes(out)

    @staticmethod
    def from_compressed(data: bytes) -> "G1Affine":
        """the inverse of to_compressed (host integers: y = (x^3 + 4)^((p + 1) / 4), the sign from bit 5); raises ValueError on
        an encoding that is not compressed, not canonical or not on the curve"""
        if len(data) != 48 or not data[0] & 0x80:
            raise ValueError("not a 48-byte compressed G1 encoding")
        if data[0] & 0x40:
            if data[0] != 0xC0 or any(data[1:]):
                raise ValueError("a non-canonical encoding of the identity")
            return G1Affine.identity()
        x = int.from_bytes(bytes([data[0] & 0x1F]) + data[1:], "big")
        if x >= P:
            raise ValueError("x is not reduced")
        rhs = (x * x * x + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P != rhs:
            raise ValueError("not on the curve")
        if bool(data[0] & 0x20) != (y > (P - 1) // 2):
            y = P - y
        return G1Affine.from_ints(x, y)

    def __eq__(self, other) -> bool:
        return isinstance(other, G1Affine) and self.limbs == other.limbs

    def __hash__(self) -> int:
        return hash(self.limbs)

    def __repr__(self) -> str:
        return "G1Affine(identity)" if self.is_identity() else "G1Affine(%s)" % self.to_compressed().hex()


def points_of(t: torch.Tensor) -> list:
    """int64[k, 12] (device or host) -> k G1Affines"""
    return [G1Affine(row) for row in t.cpu().tolist()]


def points_tensor(points, device) -> torch.Tensor:
    """G1Affines -> int64[k, 12] on `device`"""
    rows = [[w - (1 << 64) if w >> 63 else w for w in p.limbs] for p in points]
    return torch.tensor(rows, dtype=torch.int64, device=device).view(len(rows), 12)


class CommitKey:
    """the powers tau^i base, i <= max_degree, as int64[max_degree + 1, 12] on the engine's device (dusk-plonk's CommitKey)"""

    def __init__(self, engine, powers: torch.Tensor):
        self.engine = engine
        self.powers = powers

    @staticmethod
    def setup(engine, max_degree: int, tau, base: G1Affine | None = None) -> "CommitKey":
        """max_degree + 1 powers of an INSECURE development SRS with the caller's secret tau (pg_srs_setup; dusk-plonk's
        PublicParameters::setup with the randomness replaced by tau).  Whoever knows tau can forge proofs."""
        from .engine import PgError, _field
        n = max_degree + 1
        if n < 1:
            raise ValueError("max_degree must be >= 0")
        out = torch.empty((n, 12), dtype=torch.int64, device=engine.device)
        b = C.byref(base.c) if base is not None else None
        st = engine._lib.pg_srs_setup(engine._h, C.byref(_field(tau).c), b, n, out.data_ptr(), engine._stream())
        if st != 0:
            raise PgError(st, "pg_srs_setup")
        return CommitKey(engine, out)

    @property
    def max_degree(self) -> int:
        return self.powers.shape[0] - 1

    def trim(self, degree: int) -> "CommitKey":
        """the key for polynomials of degree <= `degree`: a view of the first degree + 1 powers"""
        if degree > self.max_degree:
            raise PolynomialDegreeTooLarge(f"degree {degree} > the key's {self.max_degree}")
        return CommitKey(self.engine, self.powers[:degree + 1])

    def commit(self, polys: torch.Tensor):
        """sum_i c_i tau^i base for a polynomial int64[n, 4] (-> one G1Affine) or several int64[c, n, 4] (-> a list), coefficients
        on the device in Montgomery form; n may be anything up to the key's length"""
        n = polys.shape[-2]
        if n > self.powers.shape[0]:
            raise PolynomialDegreeTooLarge(f"a polynomial of {n} coefficients > the key's {self.powers.shape[0]} powers")
        out = self.engine.msm(self.powers[:n], polys)
        return out[0] if polys.dim() == 2 else out

    def aggregate_witness(self, polys, point, v):
        """dusk-plonk's CommitKey::compute_aggregate_witness then ruffini: the opening witness of sum_j v^j p_j at `point`
        (Engine.open with mu_j = v^j) -> (witness int64[n, 4], the combination's value at point)"""
        from .engine import _field
        c = polys.shape[0] if isinstance(polys, torch.Tensor) and polys.dim() == 3 else len(polys)
        vv, mu = _field(v), []
        for j in range(c):
            mu.append(_field(1) if j == 0 else mu[-1] * vv)
        return self.engine.open(polys, mu, point)
