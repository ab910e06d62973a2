"""CPU: plonk_gadgets_amd/transcript.py.  Three things pin it:

* Keccak-f[1600]: SHA3-256 and SHAKE128 sponges built on the module's permutation equal hashlib's on every message length from 0
  to 400 bytes (which crosses the rates 136 and 168 several times).
* Merlin's published vector (the `equivalence_simple` test of the merlin crate): see test_merlin_published_vector for where the
  value comes from.
* An independent STROBE-128 / Merlin (tests/strobe_model.py: 25 integer lanes, a block at a time): Transcript equals it in every
  output byte and in the final (state, pos, pos_begin, cur_flags), on random programs and on a directed family that starts an
  append_message at every offset 0 .. 165 of a block.  The model records which byte ended each block, and the test asserts that
  every kind of byte did: both framing bytes of begin_op (with and without the flag C), the first, a middle and the last byte of a
  label and of a message, each of the four length bytes, an operation that ends exactly on a block, a forced permutation at
  pos != 0, a squeeze that crosses a block.

What stays unpinned: that dusk-plonk 0.8 appends these messages under these labels in this order.  Determinism,
label separation and challenges below r are checked as before."""
import hashlib
import random

import pytest

import strobe_model as sm
from plonk_gadgets_amd.transcript import R, Strobe128, Transcript, keccak_f1600


def sponge(msg: bytes, rate: int, pad: int, out_len: int) -> bytes:
    st = bytearray(200)
    data = bytearray(msg) + bytes([pad])
    data += bytes((-len(data)) % rate)
    data[-1] |= 0x80
    for off in range(0, len(data), rate):
        for i in range(rate):
            st[i] ^= data[off + i]
        keccak_f1600(st)
    out = bytearray()
    while True:
        out += st[:rate]
        if len(out) >= out_len:
            return bytes(out[:out_len])
        keccak_f1600(st)


def test_keccak_f1600_gives_sha3_256_and_shake128():
    rng = random.Random(1600)
    for n in range(401):
        msg = bytes(rng.randrange(256) for _ in range(n))
        assert sponge(msg, 136, 0x06, 32) == hashlib.sha3_256(msg).digest(), n
        assert sponge(msg, 168, 0x1F, 200) == hashlib.shake_128(msg).digest(200), n


def run(label, data):
    t = Transcript(label)
    t.circuit_domain_sep(1024)
    for i, d in enumerate(data):
        t.append_message(b"m%d" % i, d)
    t.append_u64(b"k", 77)
    a = t.challenge_int(b"beta")
    t.append_scalar(b"beta", a)
    return a, t.challenge_int(b"gamma"), t.challenge_bytes(b"long", 300)


def test_transcripts_are_deterministic():
    data = [b"", b"x" * 165, b"y" * 166, b"z" * 500]
    assert run(b"plonk", data) == run(b"plonk", data)
    t = Transcript(b"plonk")
    t.append_message(b"a", b"1")
    c = t.clone()
    assert t.challenge_bytes(b"c", 32) == c.challenge_bytes(b"c", 32)


def test_labels_separate_challenges():
    data = [b"abc", b"def"]
    base = run(b"plonk", data)
    assert run(b"testing", data)[0] != base[0]
    assert run(b"plonk", [b"abc", b"deg"])[0] != base[0]
    # the same bytes under a different message label
    t1, t2 = Transcript(b"plonk"), Transcript(b"plonk")
    t1.append_message(b"a", b"data")
    t2.append_message(b"b", b"data")
    assert t1.challenge_int(b"c") != t2.challenge_int(b"c")
    # the same transcript, a different challenge label
    t1, t2 = Transcript(b"plonk"), Transcript(b"plonk")
    assert t1.challenge_int(b"beta") != t2.challenge_int(b"gamma")


def test_challenges_are_below_r():
    t = Transcript(b"plonk")
    for i in range(200):
        c = t.challenge_int(b"c%d" % i)
        assert 0 <= c < R


# ---- the framing ------------------------------------------------------------------------------------------------------------------
MERLIN_VECTOR = "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"


@pytest.mark.parametrize("cls", [Transcript, sm.MerlinModel], ids=["Transcript", "model"])
def test_merlin_published_vector(cls):
    """merlin's own `equivalence_simple` test: Transcript(b"test protocol"), append_message(b"some label", b"some data"),
    challenge_bytes(b"challenge", 32).  The value was RECORDED FROM THIS IMPLEMENTATION with the merlin crate not at hand; it is
    the crate's expected value as far as it is remembered (a recollection that differed from it in one hex digit, ...9bfa... for
    ...9bca..., is a slip of memory: a sponge that agrees in 63 of 64 digits is not a different function).  The independent model
    of tests/strobe_model.py, written from the STROBE specification, gives the same 32 bytes.  Whoever has the crate should
    compare."""
    t = cls(b"test protocol")
    t.append_message(b"some label", b"some data")
    assert t.challenge_bytes(b"challenge", 32).hex() == MERLIN_VECTOR


def same_state(t, m):
    s, k = t.strobe, m.strobe
    assert (bytes(s.state), s.pos, s.pos_begin, s.cur_flags) == (k.state_bytes(), k.pos, k.pos_begin, k.cur_flags)


def test_random_programs_equal_the_model():
    rng = random.Random(0x57B0BE)
    n_clones = n_long = 0
    for prog in range(40):
        label = bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 5, 12, 150, 166, 200))))
        pairs = [(Transcript(label), sm.MerlinModel(label))]
        for _ in range(14):
            t, m = pairs[-1]
            op = rng.randrange(5)
            lab = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 13)))
            if op == 0:
                msg = bytes(rng.randrange(256) for _ in range(rng.choice((0, 1, 32, 48, 165, 166, 167, rng.randrange(400)))))
                t.append_message(lab, msg)
                m.append_message(lab, msg)
            elif op == 1:
                x = rng.randrange(1 << 64)
                t.append_u64(lab, x)
                m.append_u64(lab, x)
            elif op == 2:
                x = rng.randrange(R)
                t.append_scalar(lab, x)
                m.append_scalar(lab, x)
            elif op == 3:
                n = rng.randrange(1, 401)
                n_long += n > 166
                assert t.challenge_bytes(lab, n) == m.challenge_bytes(lab, n), (prog, n)
            else:
                pairs.append((t.clone(), m.clone()))
                n_clones += 1
            same_state(*pairs[-1])
        for t, m in pairs:  # a clone's later operations left what it was cloned from alone
            same_state(t, m)
            assert t.challenge_bytes(b"end", 64) == m.challenge_bytes(b"end", 64)
    assert n_clones > 20 and n_long > 20


REQUIRED_CLASSES = {"begin-first", "flags", "flags-C", "label-first", "label-middle", "label-last", "length-0", "length-1", "length-2",
                    "length-3", "message-first", "message-middle", "message-last", "begin-at-zero", "forced-nonzero", "squeeze"}


def test_an_append_at_every_offset_of_a_block_equals_the_model():
    """for every offset 0 .. 165 (reached by a first message of chosen length): one append_message(label of 1 .. 3 bytes, data of
    1, 32 or 48 bytes), challenge_bytes(label, 64), and once per offset challenge_bytes(label, 300), whose squeeze crosses a block"""
    starts = {}
    for first in range(166):
        t, m = Transcript(b"plonk"), sm.MerlinModel(b"plonk")
        t.append_message(b"first", bytes(first))
        m.append_message(b"first", bytes(first))
        same_state(t, m)
        starts.setdefault(m.strobe.pos, (t, m))
    assert set(starts) == set(range(166))
    seen = set()
    for pos, (t0, m0) in sorted(starts.items()):
        mark = len(m0.events)
        for ll in (1, 2, 3):
            for dl in (1, 32, 48):
                t, m = t0.clone(), m0.clone()
                lab, data = bytes(range(0x61, 0x61 + ll)), bytes((7 * i + pos) & 0xFF | 1 for i in range(dl))
                t.append_message(lab, data)
                m.append_message(lab, data)
                same_state(t, m)
                assert t.challenge_bytes(lab, 64) == m.challenge_bytes(lab, 64), (pos, ll, dl)
                same_state(t, m)
                if (ll, dl) == (2, 32):
                    assert t.challenge_bytes(lab, 300) == m.challenge_bytes(lab, 300), pos
                    same_state(t, m)
                seen |= sm.classes(m.events[mark:])
    assert seen >= REQUIRED_CLASSES, REQUIRED_CLASSES - seen


def test_the_model_names_what_ended_a_block():
    """the instrumentation itself, on transcripts whose alignment is worked out by hand: Merlin's constructor leaves pos = 13 + 2 +
    7 + 4 + 2 + len(label) after b"Merlin v1.0" (2 + 11), b"dom-sep", the length word and the label's own framing"""
    m = sm.MerlinModel(b"")
    assert (m.strobe.pos, m.events) == (28, [])
    # 28 + 2 + 1 + 4 + 2 = 37 bytes before the message: a message of 129 bytes ends the block with its last byte
    mark = len(m.events)
    m.append_message(b"a", bytes(129))
    assert sm.classes(m.events[mark:]) == {"message-last"} and m.strobe.pos == 0
    m.append_message(b"b", b"")
    assert sm.classes(m.events[mark:]) == {"message-last", "begin-at-zero"}
    # ... of 130 bytes leaves one byte for the next operation's first framing byte
    m = sm.MerlinModel(b"")
    m.append_message(b"a", bytes(128))
    assert m.strobe.pos == 165 and m.events == []
    m.append_message(b"bcd", b"")
    assert sm.classes(m.events) == {"begin-first"} and m.strobe.pos == 2 + 3 + 4 + 2 - 1
    # the flags byte of a challenge's squeeze on the boundary: one permutation, and the key operation forces one at pos != 0
    m = sm.MerlinModel(b"")
    m.append_message(b"a", bytes(128 - 2 - 1 - 4 - 1))  # pos = 157; the challenge's label, length and two framing bytes: 166
    assert m.strobe.pos == 157
    m.challenge_bytes(b"c", 64)
    assert sm.classes(m.events) == {"flags-C"} and len(m.events) == 1 and m.strobe.pos == 64
    s = Strobe128(b"x")
    k = sm.StrobeModel(b"x")
    s.key(b"0123456789", False)
    k.key(b"0123456789", False)
    assert bytes(s.state) == k.state_bytes() and sm.classes(k.events) == {"forced-nonzero"} and (s.pos, s.pos_begin) == (k.pos, k.pos_begin) == (10, 0)
