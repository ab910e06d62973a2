"""What the tests of pg_plonk_sides share: synthetic verifier keys and proofs (not sound -- commitments are k G, evaluations random
reduced scalars), the rejected encodings, the call of pg_plonk_sides_host through ctypes, and the comparison of its 23 rows with
verifier.sides' {point: [a, b]} table."""
import ctypes as C
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import g1_codec_model as M  # noqa: E402
import g1_model as G  # noqa: E402

import plonk_gadgets_amd as pg  # noqa: E402
from plonk_gadgets_amd import _lib  # noqa: E402
from plonk_gadgets_amd import verifier as V  # noqa: E402
from plonk_gadgets_amd.proof import COMMITMENTS, EVALUATIONS  # noqa: E402

R = G.R_FR
MASK = (1 << 64) - 1
RINV = pow(1 << 256, -1, R)
ROWS, PROOF = V.SIDES_ROWS, V.PROOF_BYTES
EVAL_AT = 48 * len(COMMITMENTS)
LABELS = (b"plonk", b"", bytes(range(150)), bytes(200 - i for i in range(200)))
# a label of every length 0 .. 165: together they leave a key's seed at every position 0 .. 165 of the sponge's block
SEED_LABELS = tuple(bytes((37 * i + 11 * n + 1) & 0xFF for i in range(n)) for n in range(166))


class Ok:
    """an opening key as far as sides and VerifierKey.record read it"""
    g = pg.G1Affine.generator()


def point(k):
    pt = G.mul(k, G.G)
    return pg.G1Affine.identity() if pt is None else pg.G1Affine.from_ints(*pt)


def make_key(n, seed):
    rng = random.Random(seed)
    return pg.VerifierKey(n, {name: point(rng.randrange(1, 1 << 40)) for name in pg.VerifierKey.NAMES})


def make_proof(seed):
    """the fourth wire's commitment is the identity and two commitments are equal, as a prover's can be"""
    rng = random.Random(seed)
    ks = [rng.randrange(1, 1 << 40) for _ in COMMITMENTS]
    ks[3] = 0
    ks[2] = ks[1]
    return pg.Proof(*[point(k) for k in ks], *[pg.BlsScalar.from_int(rng.randrange(R)) for _ in EVALUATIONS])


def seed_position_batch():
    """one key of n = 2^12, one proof, public inputs on two rows, and the key's 166 records under SEED_LABELS: proof i of the batch
    goes under record i -> (vk, proof bytes, public inputs, records)"""
    vk = make_key(1 << 12, 0x5EED)
    pi = {3: 0x1234_5678_9abc_def0, (1 << 12) - 1: R - 5}
    return vk, make_proof(0x5EEE).to_bytes(), pi, [vk.record(Ok, lab) for lab in SEED_LABELS]


def spread_rows(n: int, count: int, salt: int) -> dict:
    """public inputs on `count` distinct rows of [0, n) -- the first and the last among them -- or on all n rows if n < count"""
    count = min(count, n)
    rows = {0, n - 1} if count > 1 else {0}
    k = 0
    while len(rows) < count:
        rows.add((salt * 0x9E3779B97F4A7C15 + k * 0xD1B54A32D192ED03) % n)
        k += 1
    return {r: pow(7, salt + j + 1, R) for j, r in enumerate(sorted(rows)[:count])} if count else {}


def extreme_batch(n_proofs=70):
    """the smallest and the largest circuit (n = 1: log2 n = 0; n = 2^32: the largest pg_plonk_sides accepts) and n = 2^12,
    interleaved, with ragged public inputs of 0, 1, 64 and 257 rows (n = 1 has the one row) across the lanes of a workgroup
    -> (proof bytes, records, key indices, public inputs, [(vk, label)] per record)"""
    keyed = [(make_key(1, 0xE0), SEED_LABELS[165]), (make_key(1 << 32, 0xE1), SEED_LABELS[137]), (make_key(1 << 12, 0xE2), LABELS[0])]
    proofs = [make_proof(0xE10 + i).to_bytes() for i in range(3)]
    index = [i % 3 for i in range(n_proofs)]
    pis = [spread_rows(keyed[index[i]][0].n, (257, 64, 1, 0)[(i // 3) % 4], i) or None for i in range(n_proofs)]
    assert {len(p or {}) for p in pis} == {0, 1, 64, 257}
    return b"".join(proofs[(i // 4) % 3] for i in range(n_proofs)), [vk.record(Ok, lab) for vk, lab in keyed], index, pis, keyed


def with_commitment(data: bytes, j: int, enc: bytes) -> bytes:
    return data[:48 * j] + enc + data[48 * j + 48:]


def with_evaluation(data: bytes, k: int, value: int) -> bytes:
    return data[:EVAL_AT + 32 * k] + value.to_bytes(32, "little") + data[EVAL_AT + 32 * k + 32:]


def rejected_encodings():
    """name -> (48 bytes, the PG_G1_* status they decode to)"""
    good = G.compressed(G.mul(5, G.G))
    x = 1
    while pow(x * x * x + 4, (G.P - 1) // 2, G.P) == 1:
        x += 1
    outside = G.compressed(M.curve_point_from_x(random.Random(0x0f)))
    out = {"compressed-bit-clear": (bytes([good[0] & 0x7F]) + good[1:], M.BAD_ENCODING), "x-not-below-p": (M.raw_x(G.P, 0x80), M.BAD_ENCODING),
           "x-with-no-y": (M.raw_x(x, 0x80), M.NOT_ON_CURVE), "outside-the-subgroup": (outside, M.NOT_IN_SUBGROUP)}
    for enc, st in out.values():
        assert M.decode(enc)[1] == st
    return out


def model_sides(data: bytes, vk, public_inputs, label):
    """verifier.sides on a proof given as bytes; None also when the bytes are no Proof at all"""
    try:
        proof = pg.Proof.from_bytes(data)
    except ValueError:
        return None
    return V.sides(proof, vk, Ok, public_inputs, label)


def csr(pis):
    """public inputs [{row: int}] -> (offsets, rows, the values' Montgomery limbs, flat)"""
    off, rows, vals = [0], [], []
    for pi in pis:
        for row, v in (pi or {}).items():
            rows.append(row)
            m = (v % R << 256) % R
            vals.extend((m >> (64 * i)) & MASK for i in range(4))
        off.append(len(rows))
    return off, rows, vals


def host_sides(data: bytes, records, key_index=None, pis=None, col_stride=None, fill=0):
    """pg_plonk_sides_host -> (bases, scalars, status, where) as the raw bytes of the four outputs and the call's return"""
    lib = _lib.load()
    n = len(data) // PROOF
    stride = ROWS * n if col_stride is None else col_stride
    proofs = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    nk = len(records)
    keys = (_lib.PlonkKeyC * max(nk, 1))()
    C.memmove(keys, b"".join(records), nk * C.sizeof(_lib.PlonkKeyC))
    idx = (C.c_uint32 * n)(*key_index) if key_index is not None else None
    off = rows = vals = None
    if pis is not None:
        o, r_, v = csr(pis)
        off, rows, vals = (C.c_uint64 * len(o))(*o), (C.c_uint64 * max(len(r_), 1))(*r_), (C.c_uint64 * max(len(v), 1))(*v)
    bases = (C.c_uint64 * (12 * ROWS * n))(*([fill] * (12 * ROWS * n)))
    scalars = (C.c_uint64 * (4 * 2 * stride))(*([fill] * (8 * stride)))
    status, where = (C.c_uint8 * n)(*([0xEE] * n)), (C.c_uint8 * n)(*([0xEE] * n))
    st = lib.pg_plonk_sides_host(proofs, n, keys, nk, idx, off, rows, vals, bases, scalars, stride, status, where)
    return st, bytes(bases), bytes(scalars), bytes(status), bytes(where)


def words(raw: bytes):
    return [int.from_bytes(raw[i:i + 8], "little") for i in range(0, len(raw), 8)]


def grouped(bases: bytes, scalars: bytes, i: int, stride: int):
    """proof i's 23 rows grouped by base limbs with the scalars summed mod r, zero entries dropped: {limbs: (a, b)}"""
    b, s = words(bases), words(scalars)
    out = {}
    for row in range(ROWS * i, ROWS * i + ROWS):
        limbs = tuple(b[12 * row:12 * row + 12])
        ab = [sum(w << (64 * k) for k, w in enumerate(s[4 * (col * stride + row):4 * (col * stride + row) + 4])) * RINV % R for col in (0, 1)]
        acc = out.setdefault(limbs, [0, 0])
        acc[0], acc[1] = (acc[0] + ab[0]) % R, (acc[1] + ab[1]) % R
    return {k: tuple(v) for k, v in out.items() if any(v)}


def model_grouped(table):
    return {p.limbs: (a % R, b % R) for p, (a, b) in table.items() if a % R or b % R}


def rows_are_empty(bases: bytes, scalars: bytes, i: int, stride: int) -> bool:
    b, s = words(bases), words(scalars)
    return (not any(b[12 * ROWS * i:12 * ROWS * (i + 1)])
            and not any(any(s[4 * (col * stride + ROWS * i):4 * (col * stride + ROWS * (i + 1))]) for col in (0, 1)))
