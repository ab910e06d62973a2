"""The prover's Fiat-Shamir transcript: Merlin (STROBE-128 over Keccak-f[1600]) in pure Python, with dusk-plonk 0.8's
TranscriptProtocol on top [DEP-RECALL].  A proof feeds it a few hundred bytes, so it runs on the host.

What tests/test_transcript.py pins: the permutation (SHA3-256 and SHAKE128 sponges built on it equal hashlib's); the STROBE and
Merlin framing, by merlin's published vector and by an independent STROBE-128 (tests/strobe_model.py) that this one equals byte for
byte and state for state with a block boundary on every kind of byte; and, through tests/test_sides_replay_host.py and
tests/test_gpu_sides_replay.py, the table-driven replay of csrc/plonk_sides.hpp against this class from every seed position, on the
host and on the device.  What is still unpinned: that dusk-plonk 0.8 appends these messages under these labels in this order is a
recollection [DEP-RECALL]; no vector for it exists here."""
from __future__ import annotations

from .scalar import BlsScalar

# the scalar field's modulus r
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

_MASK = (1 << 64) - 1
_RC = (0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001,
       0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A,
       0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080,
       0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008)
# rotation offsets r[x][y] of rho
_ROT = ((0, 36, 3, 41, 18), (1, 44, 10, 45, 2), (62, 6, 43, 15, 61), (28, 55, 25, 21, 56), (27, 20, 39, 8, 14))


def _rol(v: int, s: int) -> int:
    return ((v << s) | (v >> (64 - s))) & _MASK if s else v


def keccak_f1600_lanes(a: list) -> list:
    """Keccak-f[1600] on 25 64-bit lanes, lane (x, y) at a[x + 5 y]"""
    a = list(a)
    for rc in _RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(a[x + 5 * y], _ROT[x][y])
        a = [b[i] ^ ((~b[(i % 5 + 1) % 5 + 5 * (i // 5)]) & b[(i % 5 + 2) % 5 + 5 * (i // 5)]) for i in range(25)]
        a[0] ^= rc
    return a


def keccak_f1600(state: bytearray) -> None:
    """Keccak-f[1600] in place on 200 bytes (lanes little-endian)"""
    lanes = [int.from_bytes(state[8 * i:8 * i + 8], "little") for i in range(25)]
    lanes = keccak_f1600_lanes(lanes)
    state[:] = b"".join(v.to_bytes(8, "little") for v in lanes)


# ---- STROBE-128, the subset Merlin uses (merlin's strobe.rs) --------------------------------------------------------------
_FLAG_I, _FLAG_A, _FLAG_C, _FLAG_T, _FLAG_M, _FLAG_K = 1, 2, 4, 8, 16, 32
_STROBE_R = 166


class Strobe128:
    def __init__(self, protocol_label: bytes):
        st = bytearray(200)
        st[0:6] = bytes([1, _STROBE_R + 2, 1, 0, 1, 96])
        st[6:18] = b"STROBEv1.0.2"
        keccak_f1600(st)
        self.state, self.pos, self.pos_begin, self.cur_flags = st, 0, 0, 0
        self.meta_ad(protocol_label, False)

    def clone(self) -> "Strobe128":
        c = Strobe128.__new__(Strobe128)
        c.state, c.pos, c.pos_begin, c.cur_flags = bytearray(self.state), self.pos, self.pos_begin, self.cur_flags
        return c

    def _run_f(self):
        self.state[self.pos] ^= self.pos_begin
        self.state[self.pos + 1] ^= 0x04
        self.state[_STROBE_R + 1] ^= 0x80
        keccak_f1600(self.state)
        self.pos = self.pos_begin = 0

    def _absorb(self, data: bytes):
        for b in data:
            self.state[self.pos] ^= b
            self.pos += 1
            if self.pos == _STROBE_R:
                self._run_f()

    def _overwrite(self, data: bytes):
        for b in data:
            self.state[self.pos] = b
            self.pos += 1
            if self.pos == _STROBE_R:
                self._run_f()

    def _squeeze(self, n: int) -> bytes:
        out = bytearray(n)
        for i in range(n):
            out[i] = self.state[self.pos]
            self.state[self.pos] = 0
            self.pos += 1
            if self.pos == _STROBE_R:
                self._run_f()
        return bytes(out)

    def _begin_op(self, flags: int, more: bool):
        if more:
            assert self.cur_flags == flags, "a continued operation must keep its flags"
            return
        assert not flags & _FLAG_T, "transport operations are not used"
        old_begin = self.pos_begin
        self.pos_begin = self.pos + 1
        self.cur_flags = flags
        self._absorb(bytes([old_begin, flags]))
        if flags & (_FLAG_C | _FLAG_K) and self.pos != 0:
            self._run_f()

    def meta_ad(self, data: bytes, more: bool):
        self._begin_op(_FLAG_M | _FLAG_A, more)
        self._absorb(data)

    def ad(self, data: bytes, more: bool):
        self._begin_op(_FLAG_A, more)
        self._absorb(data)

    def prf(self, n: int, more: bool) -> bytes:
        self._begin_op(_FLAG_I | _FLAG_A | _FLAG_C, more)
        return self._squeeze(n)

    def key(self, data: bytes, more: bool):
        self._begin_op(_FLAG_A | _FLAG_C, more)
        self._overwrite(data)


def _bytes(x) -> bytes:
    return x.encode() if isinstance(x, str) else bytes(x)


class Transcript:
    """merlin::Transcript with dusk-plonk 0.8's TranscriptProtocol (append_commitment, append_scalar, challenge_scalar,
    circuit_domain_sep).  Labels and messages are bytes (str is taken as UTF-8)."""

    def __init__(self, label):
        self.strobe = Strobe128(b"Merlin v1.0")
        self.append_message(b"dom-sep", label)

    def clone(self) -> "Transcript":
        t = Transcript.__new__(Transcript)
        t.strobe = self.strobe.clone()
        return t

    def append_message(self, label, message):
        message = _bytes(message)
        self.strobe.meta_ad(_bytes(label), False)
        self.strobe.meta_ad(len(message).to_bytes(4, "little"), True)
        self.strobe.ad(message, False)

    def append_u64(self, label, x: int):
        self.append_message(label, int(x).to_bytes(8, "little"))

    def challenge_bytes(self, label, n: int) -> bytes:
        self.strobe.meta_ad(_bytes(label), False)
        self.strobe.meta_ad(n.to_bytes(4, "little"), True)
        return self.strobe.prf(n, False)

    # -- TranscriptProtocol -------------------------------------------------------------------------------------------
    def append_scalar(self, label, s):
        """32 canonical little-endian bytes (BlsScalar::to_bytes)"""
        v = s.to_int() if isinstance(s, BlsScalar) else int(s) % R
        self.append_message(label, v.to_bytes(32, "little"))

    def append_commitment(self, label, point):
        """the 48-byte compressed encoding (G1Affine::to_compressed); `point` a G1Affine or those bytes"""
        self.append_message(label, point if isinstance(point, (bytes, bytearray)) else point.to_compressed())

    def challenge_int(self, label) -> int:
        """64 bytes read little-endian, reduced mod r (BlsScalar::from_bytes_wide)"""
        return int.from_bytes(self.challenge_bytes(label, 64), "little") % R

    def challenge_scalar(self, label) -> BlsScalar:
        return BlsScalar.from_int(self.challenge_int(label))

    def circuit_domain_sep(self, n: int):
        self.append_message(b"dom-sep", b"circuit_size")
        self.append_u64(b"n", n)
