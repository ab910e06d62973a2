"""GPU: Engine.plonk_sides(..., range_term=True) (pg_plonk_range_sides) equals pg_plonk_range_sides_host byte
for byte -- bases, both scalar columns, status and where -- which tests/test_plonk_range_sides_host.py compares with verifier.sides
on the host.  Batches of 1, 64 and 65 proofs (a workgroup is 64 lanes) with records that carry a live q_range and records whose
q_range is the identity in one call (keys of n = 2^12, 1 and 2^28), rejected encodings, evaluations and public inputs and a key index
past the table inside them; K.extreme_batch's keys of n = 1, 2^12 and 2^32 with public inputs of up to 257 rows; a wider col_stride whose padding keeps its fill; and one
call on a stream that is behind (tests/lagging_stream.py)."""
import pytest
import torch

import plonk_gadgets_amd as pg
import plonk_range_sides_corpus as RK
import plonk_sides_corpus as K
from lagging_stream import LATE, TARGET_MS, calibration, lagging, release
from plonk_range_sides_corpus import ROWS
from plonk_sides_corpus import R

pytestmark = pytest.mark.gpu

N_MAX = 65
KEYS = ((1 << 12, K.LABELS[2], True), (1, K.LABELS[0], False), (1 << 28, K.LABELS[3], True))  # (n, label, q_range live)


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def records():
    out = []
    for n, lab, live in KEYS:
        rec = RK.record(K.make_key(n, 0xB00 + n.bit_length()), lab)
        out.append(rec if live else RK.without_q_range(rec))
    return out


@pytest.fixture(scope="module")
def corpus():
    """(proof bytes, key records, key indices, public inputs) of 65 proofs and the host's four outputs for them"""
    recs = records()
    base = [K.make_proof(0xC00 + i).to_bytes() for i in range(5)]
    bad = [K.with_commitment(base[0], j, enc) for j, (enc, _) in zip((0, 3, 6, 10), K.rejected_encodings().values())]
    bad += [K.with_evaluation(base[1], 9, R), K.with_evaluation(base[2], 15, (1 << 256) - 1)]
    kinds = base + bad
    proofs, index, pis = [], [], []
    for i in range(N_MAX):
        proofs.append(kinds[(i * 7) % len(kinds)] if i else kinds[0])
        index.append(3 if i == 5 else i % 3)
        n = KEYS[i % 3][0]
        pis.append([None, {0: i + 1}, {r: pow(5, i + k, R) for k, r in enumerate(sorted({0, 1 % n, n - 1, n // 2, n // 3}))}, {n: 1}][i % 4]
                   if i != 2 else None)
    proofs[64] = kinds[1]  # the one lane of the second workgroup: an accepted proof
    data = b"".join(proofs)
    st, bases, scalars, status, where = RK.host_range_sides(data, recs, index, pis)
    assert st == 0 and set(status) == {0, 1, 2, 3, 5, 7, 8} and status[0] == 0 and status[64] == 0
    # accepted proofs under records of both kinds: row 23 carries q_range for one, nothing for the other
    live = [i for i in range(N_MAX) if status[i] == 0 and index[i] == 0]
    plain = [i for i in range(N_MAX) if status[i] == 0 and index[i] == 1]
    assert live and plain
    for i in live:
        base_, a, b = RK.row(bases, scalars, i, 23, ROWS * N_MAX)
        assert any(base_) and a == 0 and b != 0
    for i in plain:
        assert RK.row(bases, scalars, i, 23, ROWS * N_MAX) == ((0,) * 12, 0, 0)
    return data, recs, index, pis, (bases, scalars, status, where)


def upload(engine, n, batch):
    data, recs, index, pis = batch[:4]
    off, rows, vals = K.csr(pis[:n])
    dev = engine.device
    return (torch.frombuffer(bytearray(data[:K.PROOF * n]), dtype=torch.uint8).to(dev),
            torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).to(dev),
            torch.tensor(index[:n], dtype=torch.int32, device=dev), torch.tensor(off, dtype=torch.int64, device=dev),
            torch.tensor(rows + [0], dtype=torch.int64, device=dev)[:len(rows)],
            torch.tensor([w - (1 << 64) if w >> 63 else w for w in vals] + [0] * 4, dtype=torch.int64, device=dev)[:len(vals)].view(-1, 4))


def as_bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", [1, 64, N_MAX])
def test_device_equals_host(engine, corpus, n):
    h_bases, h_scalars, h_status, h_where = corpus[4]
    bases, scalars, status, where = engine.plonk_sides(*upload(engine, n, corpus), range_term=True)
    assert bases.shape == (ROWS * n, 12) and scalars.shape == (2, ROWS * n, 4)
    assert as_bytes(status) == h_status[:n] and as_bytes(where) == h_where[:n]
    assert as_bytes(bases) == h_bases[:96 * ROWS * n]
    for col in (0, 1):
        at = 32 * ROWS * N_MAX * col
        assert as_bytes(scalars[col]) == h_scalars[at:at + 32 * ROWS * n], col


def test_a_wider_stride_whose_padding_keeps_its_fill(engine, corpus):
    """pg_plonk_range_sides itself, into buffers filled beforehand: 65 proofs at a stride of 24 n + 5"""
    n, pad, fill = N_MAX, 5, 0x5A5A5A5A5A5A5A5A
    h_bases, h_scalars, h_status, h_where = corpus[4]
    proofs, keys, index, off, rows, vals = upload(engine, n, corpus)
    stride = ROWS * n + pad
    dev = engine.device
    bases = torch.full((ROWS * n + 1, 12), fill, dtype=torch.int64, device=dev)
    scalars = torch.full((2, stride, 4), fill, dtype=torch.int64, device=dev)
    status = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
    where = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
    args = [engine._h, proofs.data_ptr(), n, keys.data_ptr(), len(KEYS), index.data_ptr(), off.data_ptr(), rows.data_ptr(), vals.data_ptr(),
            bases.data_ptr(), scalars.data_ptr(), stride, status.data_ptr(), where.data_ptr(), engine._stream()]
    # refused with nothing written: a stride one short, n x 24 rows at 2^31, no keys
    for at, value in ((11, ROWS * n - 1), (4, 0), (3, None)):
        assert engine._lib.pg_plonk_range_sides(*[value if i == at else a for i, a in enumerate(args)]) == 2, at
    assert engine._lib.pg_plonk_range_sides(*[{2: (1 << 31) // ROWS + 1, 11: 1 << 40}.get(i, a) for i, a in enumerate(args)]) == 2
    assert engine._lib.pg_plonk_range_sides(*[0 if i == 2 else a for i, a in enumerate(args)]) == 0
    torch.cuda.synchronize()
    assert bool((bases == fill).all()) and bool((scalars == fill).all()) and bool((status == 0xEE).all())
    assert engine._lib.pg_plonk_range_sides(*args) == 0, engine._lib.pg_last_error()
    torch.cuda.synchronize()
    assert as_bytes(status[:n]) == h_status and as_bytes(where[:n]) == h_where
    assert as_bytes(bases[:ROWS * n]) == h_bases
    for col in (0, 1):
        assert as_bytes(scalars[col, :ROWS * n]) == h_scalars[32 * ROWS * n * col:32 * ROWS * n * (col + 1)], col
    assert bool((scalars[:, ROWS * n:] == fill).all()) and bool((bases[ROWS * n:] == fill).all())
    assert bool((status[n:] == 0xEE).all()) and bool((where[n:] == 0xEE).all())


def test_the_smallest_and_largest_keys_with_long_public_inputs(engine):
    """K.extreme_batch: 70 proofs under keys of log2 n = 0, 12 and 32, public inputs of 0, 1, 64 and 257 rows; the n = 2^12 key's
    record without its q_range"""
    data, _, index, pis, keyed = K.extreme_batch()
    recs = [RK.record(vk, lab) for vk, lab in keyed]
    recs[2] = RK.without_q_range(recs[2])
    assert sorted(rec[203] for rec in recs) == [0, 12, 32] and {len(p or {}) for p in pis[:64]} == {0, 1, 64, 257}
    n = len(index)
    assert n == 70
    st, h_bases, h_scalars, h_status, h_where = RK.host_range_sides(data, recs, index, pis)
    assert st == 0 and h_status == bytes(n)
    bases, scalars, status, where = engine.plonk_sides(*upload(engine, n, (data, recs, index, pis)), range_term=True)
    assert as_bytes(status) == h_status and as_bytes(where) == h_where
    assert as_bytes(bases) == h_bases and as_bytes(scalars) == h_scalars


def test_one_key_and_no_public_inputs_need_no_arrays(engine, corpus):
    data, recs = corpus[0], corpus[1]
    n = 9
    proofs, keys = upload(engine, n, corpus)[:2]
    bases, scalars, status, where = engine.plonk_sides(proofs, keys[:pg.VerifierKey.RANGE_RECORD_SIZE], range_term=True)
    st, h_bases, h_scalars, h_status, h_where = RK.host_range_sides(data[:K.PROOF * n], recs[:1])
    assert st == 0 and as_bytes(status) == h_status and as_bytes(where) == h_where
    assert as_bytes(bases) == h_bases and as_bytes(scalars) == h_scalars
    with pytest.raises(ValueError):  # 1488-byte records are not 1392-byte ones
        engine.plonk_sides(proofs, keys[:pg.VerifierKey.RANGE_RECORD_SIZE])


def test_under_a_lagging_stream(engine, corpus):
    """the call is issued while its stream still has a delay in front of it; the true proofs are copied in behind that delay and
    what the buffer holds meanwhile are other proofs (tests/test_gpu_stream_order.py's scheme)"""
    n = N_MAX
    data, recs, index, pis, expected = corpus
    stale = b"".join(data[K.PROOF * ((i + 1) % n):K.PROOF * ((i + 1) % n + 1)] for i in range(n))
    exp_stale = RK.host_range_sides(stale, recs, index, pis)[1:]
    assert all(a != b for a, b in zip(expected[:3], exp_stale[:3]))
    _, keys, idx, off, rows, vals = upload(engine, n, corpus)
    dev = engine.device
    t_true = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    t_stale = torch.frombuffer(bytearray(stale), dtype=torch.uint8).to(dev)
    buf = torch.empty_like(t_true)
    call = lambda: engine.plonk_sides(buf, keys, idx, off, rows, vals, range_term=True)
    side = torch.cuda.Stream()
    try:
        assert calibration(side)["delay_ms"] >= TARGET_MS
        # warm: the engine's scratch grows on the default stream, torch's allocator gets the side stream's blocks
        buf.copy_(t_stale)
        call()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            warm = [t.clone() for t in call()]
        torch.cuda.synchronize()
        del warm
        with torch.cuda.stream(side):
            ev = lagging(side)
            buf.copy_(t_true)
            got = [t.clone() for t in call()]
            assert not ev.query(), LATE
        torch.cuda.synchronize()
    finally:
        release()
    assert tuple(as_bytes(t) for t in got) == expected
