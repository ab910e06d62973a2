"""CPU: pg_plonk_range_sides_host -- the routine plonk_range_sides_kernel runs, on the host -- against verifier.sides(...,
range_term=True) (no GPU needed).  DESIGN section 3.21.

The proofs and keys are synthetic (tests/plonk_sides_corpus.py; its keys carry a random, live q_range).  A proof's 24 rows are
grouped by base limbs and their scalars summed mod r: the result must be the model's {point: [a, b]} table exactly.  Rows 0..22
must be pg_plonk_sides_host's bytes, and row 23 (q_range, 0, -v rho_range) is checked on its own, at the corners of rho_range."""
import ctypes as C

import pytest

import plonk_range_sides_corpus as RK
import plonk_sides_corpus as K
from plonk_range_sides_corpus import KEY_BYTES, ROWS
from plonk_sides_corpus import R, V

SIZES = (1, 1 << 12)
EV_A, EV_B, EV_C, EV_A_NEXT = (K.EVALUATIONS.index(f) for f in ("a_eval", "b_eval", "c_eval", "a_next_eval"))
IDENTITY = (0,) * 12


@pytest.fixture(scope="module")
def keys():
    return {n: K.make_key(n, 0x900 + n.bit_length()) for n in SIZES}


@pytest.fixture(scope="module")
def proofs():
    return [K.make_proof(0xA00 + i).to_bytes() for i in range(4)]


def public_inputs(n, kind):
    if kind == "none":
        return None
    rows = sorted({0, n - 1, n // 2, n // 3, (n - 1) // 5})  # (five rows; one where n = 1)
    return {r: pow(3, 200 + k, R) for k, r in enumerate(rows)}


def both_hosts(data, vk, pi, label, fill=0):
    """the 24-row routine on the key's record and the 23-row routine on the record's first 1392 bytes"""
    rec = RK.record(vk, label)
    assert len(rec) == RK.RECORD_BYTES and rec[:KEY_BYTES] == vk.record(K.Ok, label)
    pis = None if pi is None else [pi]
    return RK.host_range_sides(data, [rec], pis=pis, fill=fill), K.host_sides(data, [rec[:KEY_BYTES]], pis=pis, fill=fill)


@pytest.mark.parametrize("label", K.LABELS, ids=["plonk", "empty", "150-bytes", "200-bytes"])
@pytest.mark.parametrize("n", SIZES, ids=["n=1", "n=2^12"])
def test_rows_are_the_models_table_and_only_row_23_is_new(keys, proofs, n, label):
    vk = keys[n]
    q_range = vk.commitments["q_range"]
    assert not q_range.is_identity()
    for k, kind in enumerate(("none", "several")):
        pi = public_inputs(n, kind)
        want = RK.model_sides(proofs[k], vk, pi, label)
        assert want is not None and q_range in want
        (st, bases, scalars, status, where), (st23, bases23, scalars23, status23, where23) = both_hosts(proofs[k], vk, pi, label)
        assert (st, status, where) == (st23, status23, where23) == (0, b"\0", b"\0")
        assert RK.grouped(bases, scalars, 0, ROWS) == K.model_grouped(want)
        # rows 0..22: the 23-row routine's bytes
        assert RK.raw_rows(bases, scalars, 0, ROWS, ROWS, 23) == RK.raw_rows(bases23, scalars23, 0, 23, 23, 23)
        # row 23: the key's q_range, nothing on the [tau]_2 side, the model's entry on the other
        base, a, b = RK.row(bases, scalars, 0, 23, ROWS)
        assert base == q_range.limbs and a == 0 and b == want[q_range][1] % R and b != 0


def test_a_record_whose_q_range_is_the_identity(keys, proofs):
    """row 23 is empty and the table is the one without the term -- for a key with a live q_range whose record leaves it out, and for
    a key whose q_range is the identity"""
    vk = keys[1 << 12]
    pi = public_inputs(vk.n, "several")
    rec = RK.without_q_range(RK.record(vk))
    st, bases, scalars, status, where = RK.host_range_sides(proofs[0], [rec], pis=[pi], fill=0x77)
    assert (st, status, where) == (0, b"\0", b"\0")
    assert RK.row(bases, scalars, 0, 23, ROWS) == (IDENTITY, 0, 0)
    assert RK.grouped(bases, scalars, 0, ROWS) == K.model_grouped(RK.model_sides(proofs[0], vk, pi, b"plonk", range_term=False))
    plain = K.pg.VerifierKey(vk.n, dict(vk.commitments, q_range=K.pg.G1Affine.identity()))
    rec = RK.record(plain)
    assert rec[KEY_BYTES:] == bytes(96)
    st, bases, scalars, status, where = RK.host_range_sides(proofs[0], [rec], pis=[pi], fill=0x77)
    assert (st, status, where) == (0, b"\0", b"\0")
    assert RK.row(bases, scalars, 0, 23, ROWS) == (IDENTITY, 0, 0)
    want = RK.model_sides(proofs[0], plain, pi, b"plonk")
    assert want == RK.model_sides(proofs[0], plain, pi, b"plonk", range_term=False)
    assert RK.grouped(bases, scalars, 0, ROWS) == K.model_grouped(want)
    _, bases23, scalars23, _, _ = K.host_sides(proofs[0], [rec[:KEY_BYTES]], pis=[pi])
    assert RK.raw_rows(bases, scalars, 0, ROWS, ROWS, 23) == RK.raw_rows(bases23, scalars23, 0, 23, 23, 23)


def with_differences(data, d1, d2, d3):
    """the proof with b, c and a_next rewritten so that b - 4a = d1, c - 4b = d2 and a_next - 4c = d3 (mod r)"""
    a = int.from_bytes(data[K.EVAL_AT + 32 * EV_A:K.EVAL_AT + 32 * EV_A + 32], "little")
    b = (4 * a + d1) % R
    c = (4 * b + d2) % R
    data = K.with_evaluation(K.with_evaluation(data, EV_B, b), EV_C, c)
    return K.with_evaluation(data, EV_A_NEXT, (4 * c + d3) % R)


def delta(f):
    return f * (f - 1) * (f - 2) * (f - 3) % R


# (b - 4a, c - 4b, a_next - 4c) -> rho_range as a function of alpha
RHO_CORNERS = {
    "all-three-vanish": ((0, 3, 2), lambda al: 0),
    "all-three-vanish-at-1": ((1, 1, 1), lambda al: 0),
    "only-alpha^5": ((2, 0, 0x1234_5678_9ABC), lambda al: pow(al, 5, R) * delta(0x1234_5678_9ABC) % R),
    "b-4a=4": ((4, 1, 3), lambda al: pow(al, 3, R) * 24 % R),
    "c-4b=4": ((0, 4, 0), lambda al: pow(al, 4, R) * 24 % R),
    "a_next-4c=4": ((3, 2, 4), lambda al: pow(al, 5, R) * 24 % R),
    "b-4a=r-1": ((R - 1, 0, 0), lambda al: pow(al, 3, R) * 24 % R),  # delta(-1) = (-1)(-2)(-3)(-4)
    "a_next-4c=r-1": ((1, 2, R - 1), lambda al: pow(al, 5, R) * 24 % R),
    "all-live": ((R - 1, 4, 5), lambda al: (pow(al, 3, R) * 24 + pow(al, 4, R) * 24 + pow(al, 5, R) * 120) % R),
}


@pytest.mark.parametrize("case", list(RHO_CORNERS))
def test_rho_at_its_corners(keys, proofs, case, monkeypatch):
    """row 23's scalar is -v rho_range with rho_range what proof.range_rho gives for the proof's evaluations and the transcript's
    alpha -- both taken from the model's own call of range_rho -- and v read off rows 17 and 18 (-v^9 and -v^2)"""
    vk = keys[1 << 12]
    diffs, closed_form = RHO_CORNERS[case]
    data = with_differences(proofs[1], *diffs)
    calls = []
    real = V.range_rho

    def recording(ev, alpha):
        calls.append((dict(ev), alpha, real(ev, alpha)))
        return calls[-1][2]
    monkeypatch.setattr(V, "range_rho", recording)
    want = RK.model_sides(data, vk, None, b"plonk")
    assert want is not None and len(calls) == 1
    ev, alpha, rho = calls[0]
    assert ((ev["b_eval"] - 4 * ev["a_eval"]) % R, (ev["c_eval"] - 4 * ev["b_eval"]) % R, (ev["a_next_eval"] - 4 * ev["c_eval"]) % R) == diffs
    assert rho == closed_form(alpha) == K.pg.proof.range_rho(ev, alpha)
    st, bases, scalars, status, where = RK.host_range_sides(data, [RK.record(vk)])
    assert (st, status, where) == (0, b"\0", b"\0")
    v2, v9 = (-RK.row(bases, scalars, 0, k, ROWS)[2] % R for k in (18, 17))
    v = v9 * pow(v2, -4, R) % R
    assert v * v % R == v2
    base, a, b = RK.row(bases, scalars, 0, 23, ROWS)
    assert base == vk.commitments["q_range"].limbs and a == 0
    assert b == -v * rho % R
    assert (b == 0) == case.startswith("all-three-vanish")
    assert RK.grouped(bases, scalars, 0, ROWS) == K.model_grouped(want)


def test_rejections_are_the_23_row_routines_and_leave_24_empty_rows(keys, proofs):
    vk = keys[1 << 12]
    cases = [(K.with_commitment(proofs[0], j, enc), None) for j in (0, 4, 10) for enc, _ in K.rejected_encodings().values()]
    cases += [(K.with_evaluation(proofs[1], k, R), None) for k in (0, 15)]
    cases += [(proofs[2], {vk.n: 5}), (proofs[2], {0: 1, vk.n + 7: 3})]
    seen = set()
    for data, pi in cases:
        (st, bases, scalars, status, where), (st23, _, _, status23, where23) = both_hosts(data, vk, pi, b"plonk", fill=0x77)
        assert (st, status, where) == (st23, status23, where23) and st == 0 and status != b"\0"
        assert RK.rows_are_empty(bases, scalars, 0, ROWS)
        seen.add(status[0])
    assert seen == {1, 2, 3, 5, 7}
    # a key index past the table rejects that proof alone; so does a record whose sponge position is out of range
    recs = [RK.record(keys[1]), RK.record(vk)]
    data = proofs[0] + proofs[1] + proofs[2]
    st, bases, scalars, status, where = RK.host_range_sides(data, recs, [1, 2, 0], fill=0x77)
    assert (st, status, where) == (0, b"\0\x08\0", bytes(3))
    assert K.host_sides(data, [r[:KEY_BYTES] for r in recs], [1, 2, 0])[3:] == (status, where)
    assert RK.rows_are_empty(bases, scalars, 1, 3 * ROWS)
    for i, n in ((0, 1 << 12), (2, 1)):
        assert RK.grouped(bases, scalars, i, 3 * ROWS) == K.model_grouped(RK.model_sides(data[K.PROOF * i:K.PROOF * (i + 1)], keys[n], None, b"plonk"))
    bad = bytearray(recs[1])
    bad[200] = 166
    st, bases, scalars, status, where = RK.host_range_sides(proofs[0], [bytes(bad)], fill=0x77)
    assert (st, status, where) == (0, b"\x08", b"\0") and RK.rows_are_empty(bases, scalars, 0, ROWS)


def test_a_batch_with_and_without_the_widget_at_a_wider_stride(keys, proofs):
    """records with a live and with an identity q_range in one call, ragged public inputs, and a gap the call does not write"""
    n = 6
    recs = [RK.record(keys[1 << 12], K.LABELS[2]), RK.without_q_range(RK.record(keys[1], K.LABELS[0]))]
    index = [i % 2 for i in range(n)]
    pis = [public_inputs(keys[SIZES[1 - i % 2]].n, ("none", "several")[(i // 2) % 2]) for i in range(n)]
    data = b"".join(proofs[i % 4] for i in range(n))
    stride = n * ROWS + 9
    st, bases, scalars, status, where = RK.host_range_sides(data, recs, index, pis, stride, fill=0x5A5A)
    assert st == 0 and status == bytes(n) and where == bytes(n)
    for i in range(n):
        vk, label, live = (keys[1 << 12], K.LABELS[2], True) if i % 2 == 0 else (keys[1], K.LABELS[0], False)
        want = RK.model_sides(proofs[i % 4], vk, pis[i], label, range_term=live)
        assert RK.grouped(bases, scalars, i, stride) == K.model_grouped(want), i
    s = K.words(scalars)
    assert set(s[4 * n * ROWS:4 * stride]) == {0x5A5A} and set(s[4 * (stride + n * ROWS):]) == {0x5A5A}


def test_argument_errors_and_the_empty_batch(keys, proofs):
    lib = K._lib.load()
    assert lib.pg_plonk_range_sides_host(None, 0, None, 0, None, None, None, None, None, None, 0, None, None) == 0
    rec = [RK.record(keys[1])]
    assert RK.host_range_sides(proofs[0], rec, col_stride=ROWS - 1)[0] == 2
    assert b"24" in lib.pg_last_error()
    assert RK.host_range_sides(proofs[0] * 3, rec, col_stride=3 * ROWS - 1)[0] == 2
    assert RK.host_range_sides(proofs[0], rec, col_stride=ROWS)[0] == 0
    assert RK.host_range_sides(proofs[0], [])[0] == 2  # n_keys = 0
    buf = (C.c_uint8 * 8192)()
    good = [buf, 1, buf, 1, None, None, None, None, buf, buf, ROWS, buf, buf]
    for at in (0, 2, 8, 9, 11, 12):  # proofs, keys, bases, scalars, status, where
        assert lib.pg_plonk_range_sides_host(*[None if i == at else x for i, x in enumerate(good)]) == 2, at
    assert lib.pg_plonk_range_sides_host(buf, 1, buf, 1, None, buf, None, None, buf, buf, ROWS, buf, buf) == 2  # offsets without rows


def test_the_record_is_the_key_record_and_q_range(keys):
    vk = keys[1 << 12]
    rec = K._lib.PlonkRangeKeyC.from_buffer_copy(RK.record(vk, b"some label"))
    assert bytes(rec)[:KEY_BYTES] == vk.record(K.Ok, b"some label")
    assert tuple(list(rec.q_range.x) + list(rec.q_range.y)) == vk.commitments["q_range"].limbs
    assert C.sizeof(K._lib.PlonkRangeKeyC) == K.pg.VerifierKey.RANGE_RECORD_SIZE == 1488
    assert K._lib.PlonkRangeKeyC.q_range.offset == 1392
