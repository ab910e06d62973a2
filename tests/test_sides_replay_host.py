"""CPU: the transcript replay of csrc/plonk_sides.hpp alone (sides_challenges<1>, through the test-only harness
tests/cpp/sides_device_ops.hip) from a seed at EVERY sponge position, against Python's Transcript set to the same seed: all seven
challenges of all 332 seeds of tests/sides_replay_corpus.py.  And fr_from_wide, the one field routine that multiplies an operand
that is not below r, against (lo + 2^256 hi) mod r in Python integers on the edges of both halves.  No GPU needed: the harness's
host functions run the code the kernels run."""
import ctypes as C

import sides_replay_corpus as K
import strobe_model as sm


def replay_host(proofs, states, pos, begin):
    n = len(pos)
    out = (C.c_uint8 * (32 * K.CHALLENGES * n))(*([0xEE] * (32 * K.CHALLENGES * n)))
    assert K.harness().sides_replay_host(proofs, n, states, pos, begin, out) == 0
    return K.challenges(bytes(out))


def test_host_replay_equals_the_transcript_at_every_seed():
    proofs, states, pos, begin, want = K.corpus()
    assert {(p, b) for p, b in zip(pos, begin)} == {(p, b) for p in range(166) for b in (0, p)} and len(pos) == 332
    got = replay_host(proofs, states, pos, begin)
    bad = [(i, k) for i in range(len(want)) for k in range(K.CHALLENGES) if got[i][k] != want[i][k]]
    assert not bad, f"{len(bad)} challenges differ, first (lane, challenge) {bad[0]}: seed {K.SEEDS[bad[0][0]]}"
    # no two lanes agree: the seed (0, 0) is there twice, but over different proofs
    assert len(set(want)) == len(want) and len({c for w in want for c in w}) == K.CHALLENGES * len(want)


def test_the_models_seeds_put_a_block_boundary_on_every_kind_of_byte():
    """what the 332 seeds are for: over them the block that phase 0 ends falls on every class of byte the table's operations
    have.  Counted with the instrumented model over verifier.sides' first four appends and the first challenge, from each pos."""
    seen = set()
    for pos in range(166):
        for begin in (0, pos):
            tr = sm.MerlinModel(b"")
            s = tr.strobe
            s.pos, s.pos_begin, s.cur_flags = pos, begin, 2
            mark = len(tr.events)
            for lab in (b"w_l", b"w_r", b"w_o", b"w_4"):
                tr.append_message(lab, bytes(48))
            tr.challenge_bytes(b"beta", 64)
            seen |= sm.classes(tr.events[mark:])
    assert seen >= {"begin-first", "flags", "flags-C", "label-first", "label-middle", "label-last", "length-0", "length-1", "length-2",
                    "length-3", "message-first", "message-middle", "message-last", "begin-at-zero", "forced-nonzero"}, seen


def test_a_seed_out_of_range_is_not_replayed():
    proofs, states, _, _, _ = K.lanes([0, 1, 2])
    got = replay_host(proofs, states, bytes([166, 5, 255]), bytes([0, 167, 0]))
    assert all(limbs == (2**64 - 1,) * 4 for lane in got for limbs in lane)


def test_fr_from_wide_on_the_host():
    pairs = K.wide_pairs()
    n = len(pairs)
    out = (C.c_uint8 * (32 * n))()
    assert K.harness().fr_from_wide_host(K.raw256(p[0] for p in pairs), K.raw256(p[1] for p in pairs), out, n) == 0
    got, want = K.limbs256(bytes(out)), K.wide_expected(pairs)
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, f"{len(bad)} of {n} differ, first lo = {hex(pairs[bad[0]][0])}, hi = {hex(pairs[bad[0]][1])}"
    assert n == 19 * 19 + (1 << 14)
