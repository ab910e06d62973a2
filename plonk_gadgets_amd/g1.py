"""BLS12-381 G1 on the host side of the commitments: G1Affine (the ABI's pg_g1_affine), CommitKey (the powers tau^i G of an
insecure development SRS or of a key loaded from bytes, on the device) and PolynomialDegreeTooLarge.  The arithmetic runs in
libplonk_gadgets_hip.so (pg_msm, pg_srs_setup, pg_g1_to_compressed, pg_g1_decompress, pg_g1_compress); this module only
converts and moves bytes."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
_R = 1 << 384
_MASK = (1 << 64) - 1
_GX = 0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb
_GY = 0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1


# the per-point status bytes of pg_g1_decompress / pg_g1_check (include/plonk_gadgets_hip.h)
G1_STATUS = ("PG_G1_OK", "PG_G1_BAD_ENCODING", "PG_G1_NOT_ON_CURVE", "PG_G1_NOT_IN_SUBGROUP", "PG_G1_NOT_REDUCED")
# points per chunk when a key streams between a file and the device (48 MiB of encodings, 96 MiB of limbs)
LOAD_CHUNK = 1 << 20


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

    # ---- bytes: 48 per power, no header (dusk-plonk 0.8's CommitKey::to_var_bytes as recalled [DEP-RECALL]: the container's
    # parity is unpinned, the point encoding is the standard one) ---------------------------------------------------------------
    def _chunks(self, chunk: int):
        """the key's encodings, `chunk` powers at a time, as host bytes"""
        n = self.powers.shape[0]
        for start in range(0, n, chunk):
            yield self.engine.g1_compress(self.powers[start:start + chunk]).cpu().numpy().tobytes()

    def to_bytes(self) -> bytes:
        return b"".join(self._chunks(LOAD_CHUNK))

    def save(self, path, chunk: int = LOAD_CHUNK) -> None:
        with open(path, "wb") as f:
            for part in self._chunks(chunk):
                f.write(part)

    @staticmethod
    def _raise_bad(index: int, status: int):
        raise ValueError(f"power {index} of the commit key is bad: {G1_STATUS[status]}")

    @staticmethod
    def _ingest(engine, n: int, fill, check: bool, chunk: int) -> "CommitKey":
        """n powers, `chunk` at a time, through ONE pinned buffer and one device buffer on the current stream:
        fill(start, count, dst) puts the encodings of powers [start, start + count) into dst, a writable uint8 view of the
        pinned buffer.  What overlaps is the host's part with the device's: chunk k is fetched (a file read, a copy out of the
        caller's bytes) while the device still decodes chunk k - 1.  The upload of chunk k is ordered behind that decode on the
        stream; once it has completed the pinned buffer is free again and chunk k - 1's verdict is there to be read without
        waiting for anything, and only then is the decode of chunk k enqueued: the device idles for the 48-byte-per-power
        upload between two decodes, not for the fetch."""
        chunk = max(1, min(chunk, n))
        powers = torch.empty((n, 12), dtype=torch.int64, device=engine.device)
        pinned = torch.empty((48 * chunk,), dtype=torch.uint8).pin_memory()
        host = pinned.numpy()
        staged = torch.empty((48 * chunk,), dtype=torch.uint8, device=engine.device)
        uploaded = torch.cuda.Event()
        stream = torch.cuda.current_stream(engine.device)
        before = None  # (start, count, status, first_bad) of the chunk whose decode is in flight
        for start in range(0, n, chunk):
            count = min(chunk, n - start)
            fill(start, count, host[:48 * count])
            staged[:48 * count].copy_(pinned[:48 * count], non_blocking=True)
            uploaded.record(stream)
            uploaded.synchronize()
            if before is not None:
                CommitKey._settle(before)
            status, first_bad = engine._g1_decompress_into(staged[:48 * count], check, powers[start:start + count])
            before = (start, count, status, first_bad)
        CommitKey._settle(before)
        return CommitKey(engine, powers)

    @staticmethod
    def _settle(entry) -> None:
        start, count, status, first_bad = entry
        bad = int(first_bad.item())
        if bad != count:
            CommitKey._raise_bad(start + bad, int(status[bad].item()))

    @staticmethod
    def from_bytes(engine, data, check: bool = True, chunk: int = LOAD_CHUNK) -> "CommitKey":
        """the key of an SRS made elsewhere, from bytes or any buffer of them (a memoryview slice is not copied before its
        upload).  Every power is decoded on the device and, with `check`, tested for membership of the order-r subgroup;
        ValueError names the first bad power and its status.  (That the powers ARE successive powers of the opening key's tau
        is PublicParameters.is_consistent's to say.)"""
        import numpy as np
        view = memoryview(data).cast("B")
        if len(view) == 0:
            raise ValueError("an empty commit key")
        if len(view) % 48:
            raise ValueError(f"a commit key is 48 bytes per power; {len(view)} is no multiple of 48")
        src = np.frombuffer(view, dtype=np.uint8)

        def fill(start, count, dst):
            dst[:] = src[48 * start:48 * (start + count)]
        return CommitKey._ingest(engine, len(view) // 48, fill, check, chunk)

    @staticmethod
    def load(engine, path, max_degree: int | None = None, check: bool = True, chunk: int = LOAD_CHUNK, offset: int = 0) -> "CommitKey":
        """from_bytes for a file (from byte `offset` on), streamed `chunk` powers at a time through a pinned buffer: one chunk is
        read from the file while the device decodes the one before (_ingest).  With max_degree only the first max_degree + 1
        powers are read (PolynomialDegreeTooLarge if the file holds fewer)."""
        import os
        size = os.path.getsize(path) - offset
        if size <= 0:
            raise ValueError("an empty commit key")
        if size % 48:
            raise ValueError(f"a commit key is 48 bytes per power; {size} is no multiple of 48")
        n = size // 48
        if max_degree is not None:
            if max_degree < 0:
                raise ValueError("max_degree must be >= 0")
            if max_degree + 1 > n:
                raise PolynomialDegreeTooLarge(f"degree {max_degree} > the file's {n - 1}")
            n = max_degree + 1
        with open(path, "rb") as f:
            f.seek(offset)

            def fill(start, count, dst):
                if f.readinto(memoryview(dst)) != 48 * count:
                    raise ValueError(f"{path}: short read")
            return CommitKey._ingest(engine, n, fill, check, chunk)

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
