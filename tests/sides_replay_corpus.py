"""What tests/test_sides_replay_host.py and tests/test_gpu_sides_replay.py share: the harness of the transcript replay
(tests/cpp/sides_device_ops.hip), 332 seeds -- one fixed 200-byte state without a zero byte at every pos 0 .. 165, with pos_begin 0
and pos_begin = pos -- and what Python's Transcript, its Strobe128 set to the same state, pos and pos_begin, squeezes from
verifier.sides' sequence of appends and challenges (strobe_model.replay_sides) over the same 1040 bytes.  The proofs are not
proofs: one is all 0xFF, one has bytes that differ wherever two of the replay's offsets could be confused, one is random, so a wrong
offset into the proof or into the table's label blob cannot cancel out.  The model costs a few seconds and is computed once."""
import ctypes as C
import functools
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpp"))
import strobe_model as sm  # noqa: E402

from plonk_gadgets_amd.transcript import R, Transcript  # noqa: E402

PROOF, CHALLENGES, RATE = sm.PROOF_BYTES, 7, sm.RATE
STATE = bytes(1 + (89 * i + 7 * (i >> 3)) % 255 for i in range(200))
PROOFS = (bytes([0xFF]) * PROOF, bytes((131 * o + 17 * (o >> 8) + 1) & 0xFF for o in range(PROOF)),
          bytes(random.Random(0x51DE5).randrange(256) for _ in range(PROOF)))
SEEDS = [(pos, 0) for pos in range(RATE)] + [(pos, pos) for pos in range(RATE)]


def mont_limbs(x: int) -> tuple:
    m = (x << 256) % R
    return tuple((m >> (64 * i)) & ((1 << 64) - 1) for i in range(4))


@functools.lru_cache(maxsize=None)
def corpus():
    """(proof bytes, states, pos, pos_begin, expected) of the 332 replays, lane i at seed SEEDS[i] over proof PROOFS[i % 3];
    expected[i] the seven challenges as Montgomery limbs"""
    assert 0 not in STATE and len(set(STATE)) > 100
    want = []
    for i, (pos, pos_begin) in enumerate(SEEDS):
        tr = Transcript(b"")
        s = tr.strobe
        s.state, s.pos, s.pos_begin, s.cur_flags = bytearray(STATE), pos, pos_begin, 2
        want.append(tuple(mont_limbs(c) for c in sm.replay_sides(tr, PROOFS[i % 3])))
    n = len(SEEDS)
    return (b"".join(PROOFS[i % 3] for i in range(n)), STATE * n, bytes(p for p, _ in SEEDS), bytes(b for _, b in SEEDS), want)


def lanes(picks):
    """the corpus restricted to (or repeated over) the lanes `picks`"""
    proofs, states, pos, begin, want = corpus()
    return (b"".join(proofs[PROOF * i:PROOF * i + PROOF] for i in picks), b"".join(states[200 * i:200 * i + 200] for i in picks),
            bytes(pos[i] for i in picks), bytes(begin[i] for i in picks), [want[i] for i in picks])


@functools.lru_cache(maxsize=None)
def harness():
    import sides_device_build
    lib = C.CDLL(sides_device_build.build())
    P, U64, I = C.c_void_p, C.c_uint64, C.c_int
    sigs = {"sides_replay_host": [P, U64, P, P, P, P], "sides_replay_device": [P, U64, P, P, P, P, I, I],
            "fr_from_wide_host": [P, P, P, U64], "fr_from_wide_device": [P, P, P, U64, I, I]}
    for name, args in sigs.items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, I
    return lib


def challenges(raw: bytes) -> list:
    """n x 7 x 32 bytes -> [7 tuples of 4 limbs]"""
    w = [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(len(raw) // 8)]
    return [tuple(tuple(w[28 * i + 4 * k:28 * i + 4 * k + 4]) for k in range(CHALLENGES)) for i in range(len(w) // 28)]


# ---- fr_from_wide ------------------------------------------------------------------------------------------------------------------
def wide_pairs():
    """(lo, hi) below 2^256 each: all pairs of the edge values, then 2^14 random pairs"""
    edges = [0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 1 << 255, (1 << 256) - 1]
    edges += [0xFFFFFFFF << (32 * k) for k in range(8)]  # every 32-bit word all ones, one at a time
    edges += [int.from_bytes(bytes.fromhex("FFFFFFFF00000000") * 4, "big"), int.from_bytes(bytes.fromhex("00000000FFFFFFFF") * 4, "big")]
    assert all(0 <= e < 1 << 256 for e in edges) and 2 * R < 1 << 256
    rng = random.Random(0xF10E)
    return [(lo, hi) for lo in edges for hi in edges] + [(rng.randrange(1 << 256), rng.randrange(1 << 256)) for _ in range(1 << 14)]


def wide_expected(pairs) -> list:
    return [mont_limbs((lo + (hi << 256)) % R) for lo, hi in pairs]


def raw256(values) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def limbs256(raw: bytes) -> list:
    return [tuple(int.from_bytes(raw[32 * i + 8 * k:32 * i + 8 * k + 8], "little") for k in range(4)) for i in range(len(raw) // 32)]
