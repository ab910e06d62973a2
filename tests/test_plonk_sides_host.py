"""CPU: pg_plonk_sides_host -- the routine plonk_sides_kernel runs, on the host -- against verifier.sides (no GPU needed).

The proofs are synthetic (tests/plonk_sides_corpus.py).  A proof's 23 rows are grouped by base limbs and their scalars summed mod
r: the result must be the model's {point: [a, b]} exactly, zero entries ignored, in both columns.  That equality pins the
transcript too: one wrong framing byte changes every challenge and with it every scalar.  Labels of 5, 0, 150 and 200 bytes put
the seed's `pos` early, late and past a block boundary of the sponge; the labels of every length 0 .. 165 (K.SEED_LABELS) put it at
every one of the 166 positions, so that every byte of the first phase's operations ends a block under some label."""
import ctypes as C

import pytest

import plonk_sides_corpus as K
from plonk_sides_corpus import G, R, ROWS, V

SIZES = (1, 2, 1 << 12, 1 << 28)


@pytest.fixture(scope="module")
def keys():
    return {n: K.make_key(n, 0x100 + n.bit_length()) for n in SIZES}


@pytest.fixture(scope="module")
def proofs():
    return [K.make_proof(0x200 + i).to_bytes() for i in range(4)]


def public_inputs(n, kind):
    if kind == "none":
        return None
    if kind == "row-0":
        return {0: 0x1234_5678_9abc_def0}
    if kind == "row-n-1":
        return {n - 1: R - 5}
    rows = sorted({0, n - 1, n // 2, n // 3, (n - 1) // 5})  # (up to five rows; fewer where n is tiny)
    return {r: pow(3, 100 + k, R) for k, r in enumerate(rows)}


def check_accepted(data, vk, pi, label):
    want = K.model_sides(data, vk, pi, label)
    assert want is not None
    st, bases, scalars, status, where = K.host_sides(data, [vk.record(K.Ok, label)], pis=[pi])
    assert st == 0 and status == b"\0" and where == b"\0"
    assert K.grouped(bases, scalars, 0, ROWS) == K.model_grouped(want)
    return bases, scalars


@pytest.mark.parametrize("label", K.LABELS, ids=["plonk", "empty", "150-bytes", "200-bytes"])
@pytest.mark.parametrize("n", SIZES, ids=["n=1", "n=2", "n=2^12", "n=2^28"])
def test_rows_are_the_models_table(keys, proofs, n, label):
    seeds = {keys[n].record(K.Ok, lab)[200] for lab in K.LABELS}
    assert len(seeds) >= 3, seeds  # the labels do leave the seed at different positions
    for k, kind in enumerate(("none", "row-0", "row-n-1", "five-rows")):
        bases, _ = check_accepted(proofs[k], keys[n], public_inputs(n, kind), label)
        # the fixed order of the rows: the proof's commitments, the key's eleven, the generator
        b = K.words(bases)
        proof = K.pg.Proof.from_bytes(proofs[k])
        want = [getattr(proof, f) for f in K.COMMITMENTS] + [keys[n].commitments[f] for f in V.SIDES_KEY_ROWS] + [K.Ok.g]
        assert [tuple(b[12 * r:12 * r + 12]) for r in range(ROWS)] == [p.limbs for p in want]


def test_a_label_of_every_length_puts_the_seed_at_every_position():
    """166 records of one key, proof i under record i, in one call"""
    vk, proof, pi, records = K.seed_position_batch()
    assert {rec[200] for rec in records} == set(range(166))  # the seeds' pos: exactly every position
    assert len({rec[201] for rec in records}) > 100          # ... and pos_begin moves with it
    n = len(records)
    st, bases, scalars, status, where = K.host_sides(proof * n, records, list(range(n)), [pi] * n)
    assert st == 0 and status == bytes(n) and where == bytes(n)
    for i, lab in enumerate(K.SEED_LABELS):
        assert K.grouped(bases, scalars, i, ROWS * n) == K.model_grouped(K.model_sides(proof, vk, pi, lab)), len(lab)


def test_the_smallest_and_largest_keys_with_long_public_inputs():
    """n = 1 and n = 2^32 (log2 n = 0 and 32, the ends of what the routine accepts) and public inputs of 0, 1, 64 and 257 rows: the
    batch tests/test_gpu_plonk_sides.py compares the device with the host on, here the host against verifier.sides"""
    data, records, index, pis, keyed = K.extreme_batch()
    assert sorted(rec[203] for rec in records) == [0, 12, 32]  # log2_n
    n = len(index)
    st, bases, scalars, status, where = K.host_sides(data, records, index, pis)
    assert st == 0 and status == bytes(n) and where == bytes(n)
    for i in range(n):
        vk, lab = keyed[index[i]]
        want = K.model_sides(data[K.PROOF * i:K.PROOF * (i + 1)], vk, pis[i], lab)
        assert K.grouped(bases, scalars, i, ROWS * n) == K.model_grouped(want), (i, vk.n, len(pis[i] or {}))


def test_a_batch_with_mixed_keys_ragged_inputs_and_a_wider_stride(keys, proofs):
    ns = [SIZES[i % 4] for i in range(7)]
    labels = [K.LABELS[(i // 2) % 4] for i in range(7)]
    pis = [public_inputs(n, ("none", "five-rows", "row-0")[i % 3]) for i, n in enumerate(ns)]
    table, records, index = {}, [], []
    for n, lab in zip(ns, labels):
        if (n, lab) not in table:
            table[n, lab] = len(records)
            records.append(keys[n].record(K.Ok, lab))
        index.append(table[n, lab])
    data = b"".join(proofs[i % 4] for i in range(7))
    stride = 7 * ROWS + 9
    st, bases, scalars, status, where = K.host_sides(data, records, index, pis, stride, fill=0x5A5A)
    assert st == 0 and status == bytes(7) and where == bytes(7)
    for i in range(7):
        want = K.model_sides(proofs[i % 4], keys[ns[i]], pis[i], labels[i])
        assert K.grouped(bases, scalars, i, stride) == K.model_grouped(want), i
    s = K.words(scalars)
    assert set(s[4 * 7 * ROWS:4 * stride]) == {0x5A5A} and set(s[4 * (stride + 7 * ROWS):]) == {0x5A5A}  # the gap is not written


@pytest.mark.parametrize("j", [0, 4, 10], ids=["a_comm", "z_comm", "w_zw_comm"])
def test_rejected_commitments(keys, proofs, j):
    vk = keys[1 << 12]
    rec = [vk.record(K.Ok)]
    for name, (enc, code) in K.rejected_encodings().items():
        data = K.with_commitment(proofs[0], j, enc)
        assert K.model_sides(data, vk, None, b"plonk") is None, name
        st, bases, scalars, status, where = K.host_sides(data, rec, fill=0x77)
        assert (st, status[0], where[0]) == (0, code, j), name
        assert K.rows_are_empty(bases, scalars, 0, ROWS), name
    # the FIRST bad commitment is the one reported
    (e1, c1), (e2, _) = (K.rejected_encodings()[k] for k in ("x-with-no-y", "compressed-bit-clear"))
    if j < 10:
        data = K.with_commitment(K.with_commitment(proofs[0], 10, e2), j, e1)
        assert K.host_sides(data, rec)[3:] == (bytes([c1]), bytes([j]))


@pytest.mark.parametrize("value", [R, (1 << 256) - 1], ids=["r", "2^256-1"])
def test_rejected_evaluations(keys, proofs, value):
    vk = keys[1 << 12]
    for k in (0, 7, 15):
        data = K.with_evaluation(proofs[1], k, value)
        assert K.model_sides(data, vk, None, b"plonk") is None
        st, bases, scalars, status, where = K.host_sides(data, [vk.record(K.Ok)], fill=0x77)
        assert (st, status[0], where[0]) == (0, 5, k)
        assert K.rows_are_empty(bases, scalars, 0, ROWS)
    # r - 1 is an evaluation like any other
    check_accepted(K.with_evaluation(proofs[1], 3, R - 1), vk, None, b"plonk")
    # a bad commitment is reported before a bad evaluation
    data = K.with_commitment(K.with_evaluation(proofs[1], 0, value), 2, K.rejected_encodings()["x-not-below-p"][0])
    assert K.host_sides(data, [vk.record(K.Ok)])[3:] == (b"\x01", b"\x02")


def test_public_input_rows_and_key_indices_out_of_range(keys, proofs):
    for n in (2, 1 << 12):
        vk = keys[n]
        rec = [vk.record(K.Ok)]
        for pi in ({n: 5}, {0: 1, n - 1: 2, n + 7: 3}, {1 << 63: 1}):
            st, bases, scalars, status, where = K.host_sides(proofs[2], rec, pis=[pi], fill=0x77)
            assert (st, status, where) == (0, b"\x07", b"\0"), (n, pi)
            assert K.rows_are_empty(bases, scalars, 0, ROWS)
    # a key index past the table rejects that proof alone
    rec = [keys[2].record(K.Ok), keys[1 << 12].record(K.Ok)]
    st, bases, scalars, status, where = K.host_sides(proofs[0] + proofs[1] + proofs[2], rec, [1, 2, 0], fill=0x77)
    assert (st, status, where) == (0, b"\0\x08\0", bytes(3))
    assert K.rows_are_empty(bases, scalars, 1, 3 * ROWS)
    for i, n in ((0, 1 << 12), (2, 2)):
        assert K.grouped(bases, scalars, i, 3 * ROWS) == K.model_grouped(K.model_sides(proofs[i], keys[n], None, b"plonk"))
    # ... and so does a key record whose sponge position is out of range
    bad = bytearray(rec[0])
    bad[200] = 166
    assert K.host_sides(proofs[0], [bytes(bad)])[3] == b"\x08"


def test_argument_errors_and_the_empty_batch(keys, proofs):
    lib = K._lib.load()
    assert lib.pg_plonk_sides_host(None, 0, None, 0, None, None, None, None, None, None, 0, None, None) == 0
    rec = [keys[2].record(K.Ok)]
    assert K.host_sides(proofs[0], rec, col_stride=ROWS - 1)[0] == 2
    assert K.host_sides(proofs[0], [])[0] == 2
    buf = (C.c_uint8 * 4096)()
    assert lib.pg_plonk_sides_host(None, 1, buf, 1, None, None, None, None, buf, buf, ROWS, buf, buf) == 2
    assert lib.pg_plonk_sides_host(buf, 1, buf, 1, None, buf, None, None, buf, buf, ROWS, buf, buf) == 2  # offsets without rows


def test_the_record_is_the_transcripts_state(keys):
    """VerifierKey.record: the seed is Transcript's state after the label, the domain separator and the 15 commitments, kept per
    label; log2 n and omega are the domain's"""
    vk = keys[1 << 12]
    rec = K._lib.PlonkKeyC.from_buffer_copy(vk.record(K.Ok, b"some label"))
    tr = K.pg.Transcript(b"some label")
    tr.circuit_domain_sep(vk.n)
    for name in vk.NAMES:
        tr.append_commitment(name.encode(), vk.commitments[name])
    s = tr.strobe
    assert (bytes(rec.state), rec.pos, rec.pos_begin, rec.cur_flags) == (bytes(s.state), s.pos, s.pos_begin, s.cur_flags)
    assert rec.log2_n == 12 and list(rec.omega.l) == K.pg.engine.domain_generator(12).limbs()
    assert [tuple(list(p.x) + list(p.y)) for p in rec.points] == [vk.commitments[f].limbs for f in V.SIDES_KEY_ROWS]
    assert tuple(list(rec.g.x) + list(rec.g.y)) == K.Ok.g.limbs
    assert b"some label" in vk._seeds and vk.record(K.Ok, b"some label") == bytes(rec)
    assert len(bytes(rec)) == K.pg.VerifierKey.RECORD_SIZE == 1392 and G.P
