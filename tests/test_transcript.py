"""CPU: plonk_gadgets_amd/transcript.py.  Keccak-f[1600] is pinned by building SHA3-256 and SHAKE128 sponges on the module's
permutation and comparing them with hashlib on every message length from 0 to 400 bytes (which crosses the rates 136 and 168
several times).  The STROBE / Merlin framing has no vectors here (parity unpinned): it is checked for determinism, for label
separation and for challenges below r."""
import hashlib
import random

from plonk_gadgets_amd.transcript import R, Transcript, keccak_f1600


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
