"""What the tests of pg_plonk_range_sides share, beside tests/plonk_sides_corpus.py: the call of pg_plonk_range_sides_host through
ctypes, 1488-byte records, and the grouping of a proof's 24 rows."""
import ctypes as C

import plonk_sides_corpus as K
from plonk_sides_corpus import R, RINV, _lib, pg

ROWS = 24
KEY_BYTES, RECORD_BYTES = 1392, 1488
assert (K.V.RANGE_SIDES_ROWS, pg.VerifierKey.RECORD_SIZE, pg.VerifierKey.RANGE_RECORD_SIZE) == (ROWS, KEY_BYTES, RECORD_BYTES)


def record(vk, label=b"plonk"):
    return vk.record(K.Ok, label, range_term=True)


def without_q_range(rec: bytes) -> bytes:
    """the record with the identity for q_range"""
    return rec[:KEY_BYTES] + bytes(RECORD_BYTES - KEY_BYTES)


def host_range_sides(data: bytes, records, key_index=None, pis=None, col_stride=None, fill=0):
    """pg_plonk_range_sides_host -> (return, bases, scalars, status, where), the four outputs as raw bytes (K.host_sides' shape)"""
    lib = _lib.load()
    n = len(data) // K.PROOF
    stride = ROWS * n if col_stride is None else col_stride
    proofs = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    nk = len(records)
    keys = (_lib.PlonkRangeKeyC * max(nk, 1))()
    C.memmove(keys, b"".join(records), nk * RECORD_BYTES)
    idx = (C.c_uint32 * n)(*key_index) if key_index is not None else None
    off = rows = vals = None
    if pis is not None:
        o, r_, v = K.csr(pis)
        off, rows, vals = (C.c_uint64 * len(o))(*o), (C.c_uint64 * max(len(r_), 1))(*r_), (C.c_uint64 * max(len(v), 1))(*v)
    bases = (C.c_uint64 * (12 * ROWS * n))(*([fill] * (12 * ROWS * n)))
    scalars = (C.c_uint64 * (8 * max(stride, 1)))(*([fill] * (8 * max(stride, 1))))
    status, where = (C.c_uint8 * n)(*([0xEE] * n)), (C.c_uint8 * n)(*([0xEE] * n))
    st = lib.pg_plonk_range_sides_host(proofs, n, keys, nk, idx, off, rows, vals, bases, scalars, stride, status, where)
    return st, bytes(bases), bytes(scalars)[:64 * stride], bytes(status), bytes(where)


def row(bases: bytes, scalars: bytes, i: int, k: int, stride: int, rows: int = ROWS):
    """row k of proof i: (the base's 12 limbs, a, b) with the scalars as canonical integers"""
    at = rows * i + k
    ab = [int.from_bytes(scalars[32 * (col * stride + at):32 * (col * stride + at) + 32], "little") * RINV % R for col in (0, 1)]
    return tuple(K.words(bases[96 * at:96 * at + 96])), ab[0], ab[1]


def raw_rows(bases: bytes, scalars: bytes, i: int, stride: int, rows: int, count: int) -> bytes:
    """the bytes of the first `count` rows of proof i: bases, then the two scalar columns"""
    at = rows * i
    return (bases[96 * at:96 * (at + count)] + scalars[32 * at:32 * (at + count)]
            + scalars[32 * (stride + at):32 * (stride + at + count)])


def grouped(bases: bytes, scalars: bytes, i: int, stride: int):
    """K.grouped for a table of 24 rows"""
    out = {}
    for k in range(ROWS):
        limbs, a, b = row(bases, scalars, i, k, stride)
        acc = out.setdefault(limbs, [0, 0])
        acc[0], acc[1] = (acc[0] + a) % R, (acc[1] + b) % R
    return {k: tuple(v) for k, v in out.items() if any(v)}


def rows_are_empty(bases: bytes, scalars: bytes, i: int, stride: int) -> bool:
    return not any(raw_rows(bases, scalars, i, stride, ROWS, ROWS))


def model_sides(data: bytes, vk, public_inputs, label, range_term=True):
    """verifier.sides(..., range_term) on a proof given as bytes; None also when the bytes are no Proof at all"""
    try:
        proof = pg.Proof.from_bytes(data)
    except ValueError:
        return None
    return K.V.sides(proof, vk, K.Ok, public_inputs, label, range_term=range_term)
