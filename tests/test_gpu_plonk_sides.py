"""GPU: Engine.plonk_sides (pg_plonk_sides) equals pg_plonk_sides_host byte for byte -- bases, scalars, status and where -- on the
corpus of tests/test_plonk_sides_host.py replicated to 1, 63, 64, 65 and 257 proofs (one lane short of a workgroup, one
workgroup, one lane more, several): three keys of different n and label interleaved through d_key_index, ragged public inputs,
every rejection class in every batch that has room for it, a key index past the table, and a scalar col_stride larger than 23 n.
And every argument error leaves sentinel-filled outputs untouched.  Two more batches, which tests/test_plonk_sides_host.py compares
with verifier.sides on the host: 166 proofs under the 166 records whose seeds stand at every position of the sponge's block (three
workgroups, every lane permuting at different bytes, rejected proofs among them), and the keys of n = 1 and n = 2^32 with public
inputs of up to 257 rows."""
import pytest
import torch

import plonk_gadgets_amd as pg
import plonk_sides_corpus as K
from plonk_sides_corpus import R, ROWS

pytestmark = pytest.mark.gpu

N_MAX = 257
KEYS = ((2, K.LABELS[0]), (1 << 12, K.LABELS[2]), (1 << 28, K.LABELS[3]))


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus():
    """(proof bytes, key records, key indices, public inputs) of 257 proofs and the host's four outputs for them"""
    records = [K.make_key(n, 0x300 + n.bit_length()).record(K.Ok, lab) for n, lab in KEYS]
    base = [K.make_proof(0x400 + i).to_bytes() for i in range(5)]
    bad = [K.with_commitment(base[0], j, enc) for j, (enc, _) in zip((0, 3, 6, 10), K.rejected_encodings().values())]
    bad += [K.with_evaluation(base[1], 9, R), K.with_evaluation(base[2], 15, (1 << 256) - 1)]
    kinds = base + bad
    proofs, index, pis = [], [], []
    for i in range(N_MAX):
        proofs.append(kinds[(i * 7) % len(kinds)] if i else kinds[0])
        index.append(3 if i == 5 else i % 3)
        n = KEYS[i % 3][0]
        pis.append([None, {0: i + 1}, {r: pow(5, i + k, R) for k, r in enumerate(sorted({0, 1, n - 1, n // 2, n // 3}))}, {n: 1}][i % 4]
                   if i != 2 else None)
    data = b"".join(proofs)
    st, bases, scalars, status, where = K.host_sides(data, records, index, pis)
    assert st == 0 and set(status) == {0, 1, 2, 3, 5, 7, 8} and status[0] == 0
    return data, records, index, pis, (bases, scalars, status, where)


def upload(engine, n, corpus):
    data, records, index, pis, _ = corpus
    off, rows, vals = K.csr(pis[:n])
    dev = engine.device
    return (torch.frombuffer(bytearray(data[:K.PROOF * n]), dtype=torch.uint8).to(dev),
            torch.frombuffer(bytearray(b"".join(records)), dtype=torch.uint8).to(dev),
            torch.tensor(index[:n], dtype=torch.int32, device=dev), torch.tensor(off, dtype=torch.int64, device=dev),
            torch.tensor(rows + [0], dtype=torch.int64, device=dev)[:len(rows)],
            torch.tensor([w - (1 << 64) if w >> 63 else w for w in vals] + [0] * 4, dtype=torch.int64, device=dev)[:len(vals)].view(-1, 4))


@pytest.mark.parametrize("n", [1, 63, 64, 65, N_MAX])
def test_device_equals_host(engine, corpus, n):
    h_bases, h_scalars, h_status, h_where = corpus[4]
    stride = ROWS * n + 5
    bases, scalars, status, where = engine.plonk_sides(*upload(engine, n, corpus), col_stride=stride)
    assert bytes(status.cpu().numpy()) == h_status[:n] and bytes(where.cpu().numpy()) == h_where[:n]
    assert bases.cpu().numpy().tobytes() == h_bases[:96 * ROWS * n]
    assert scalars.shape == (2, stride, 4)
    got = scalars[:, :ROWS * n].cpu().numpy()
    for col in (0, 1):
        at = 32 * ROWS * N_MAX * col
        assert got[col].tobytes() == h_scalars[at:at + 32 * ROWS * n], col


def device_equals_host(engine, batch):
    data, records, index, pis = batch
    n = len(index)
    st, h_bases, h_scalars, h_status, h_where = K.host_sides(data, records, index, pis)
    assert st == 0
    bases, scalars, status, where = engine.plonk_sides(*upload(engine, n, (data, records, index, pis, None)))
    assert bytes(status.cpu().numpy()) == h_status and bytes(where.cpu().numpy()) == h_where
    assert bases.cpu().numpy().tobytes() == h_bases
    assert scalars.cpu().numpy().tobytes() == h_scalars
    return h_status, h_where


def test_a_seed_at_every_position_in_one_launch(engine):
    """proof i under record i: workgroups of 64, 64 and 38 lanes, every lane's seed at another pos; one rejected proof of every
    class among them (those lanes skip the sponge), a public input past n and a key index past the table"""
    vk, proof, pi, records = K.seed_position_batch()
    assert {rec[200] for rec in records} == set(range(166))
    n = len(records)
    proofs, index, pis = [proof] * n, list(range(n)), [pi] * n
    enc = K.rejected_encodings()
    for lane, (j, name) in zip((5, 63, 64, 130), ((0, "compressed-bit-clear"), (3, "x-not-below-p"), (6, "x-with-no-y"), (10, "outside-the-subgroup"))):
        proofs[lane] = K.with_commitment(proof, j, enc[name][0])
    proofs[40] = K.with_evaluation(proof, 9, R)
    proofs[165] = K.with_evaluation(proof, 15, (1 << 256) - 1)
    pis[100] = {1 << 12: 1}
    index[127] = n
    status, where = device_equals_host(engine, (b"".join(proofs), records, index, pis))
    rejected = {5: (1, 0), 63: (1, 3), 64: (2, 6), 130: (3, 10), 40: (5, 9), 165: (5, 15), 100: (7, 0), 127: (8, 0)}
    assert [(status[i], where[i]) for i in range(n)] == [rejected.get(i, (0, 0)) for i in range(n)]


def test_the_smallest_and_largest_keys_with_long_public_inputs(engine):
    data, records, index, pis, _ = K.extreme_batch()
    assert sorted(rec[203] for rec in records) == [0, 12, 32] and {len(p or {}) for p in pis[:64]} == {0, 1, 64, 257}
    status, _ = device_equals_host(engine, (data, records, index, pis))
    assert status == bytes(len(index))


def test_no_public_inputs_and_one_key_need_no_arrays(engine, corpus):
    data, records, _, _, _ = corpus
    n = 9
    proofs, keys = upload(engine, n, corpus)[:2]
    bases, scalars, status, where = engine.plonk_sides(proofs, keys[:pg.VerifierKey.RECORD_SIZE])
    st, h_bases, h_scalars, h_status, h_where = K.host_sides(data[:K.PROOF * n], records[:1])
    assert st == 0 and bytes(status.cpu().numpy()) == h_status and bytes(where.cpu().numpy()) == h_where
    assert bases.cpu().numpy().tobytes() == h_bases and scalars.cpu().numpy().tobytes() == h_scalars


def test_argument_errors_leave_the_outputs_untouched(engine, corpus):
    n = 3
    proofs, keys, index, off, rows, vals = upload(engine, n, corpus)
    dev = engine.device
    SENT = 0x5A
    big = torch.full((96 * ROWS * n + 64 * ROWS * n + 2 * n + 64,), SENT, dtype=torch.uint8, device=dev)
    bases, scalars = big[:96 * ROWS * n], big[96 * ROWS * n:160 * ROWS * n]
    status, where = big[160 * ROWS * n:160 * ROWS * n + n], big[160 * ROWS * n + 16:160 * ROWS * n + 16 + n]
    p = lambda t: t.data_ptr()
    good = dict(e=engine._h, proofs=p(proofs), n=n, keys=p(keys), n_keys=3, index=p(index), off=p(off), rows=p(rows), vals=p(vals),
                bases=p(bases), scalars=p(scalars), stride=ROWS * n, status=p(status), where=p(where))
    order = ("e", "proofs", "n", "keys", "n_keys", "index", "off", "rows", "vals", "bases", "scalars", "stride", "status", "where")

    def call(**change):
        a = dict(good, **change)
        return engine._lib.pg_plonk_sides(*[a[k] for k in order], engine._stream())
    bad = [dict(e=None), dict(proofs=None), dict(proofs=good["proofs"] + 8), dict(keys=None), dict(keys=good["keys"] + 8), dict(n_keys=0),
           dict(index=good["index"] + 2), dict(rows=None), dict(vals=None), dict(off=good["off"] + 4), dict(vals=good["vals"] + 8),
           dict(bases=None), dict(bases=good["bases"] + 8), dict(scalars=None), dict(scalars=good["scalars"] + 8), dict(stride=ROWS * n - 1),
           dict(status=None), dict(where=None), dict(where=good["status"]), dict(status=good["bases"] + 96), dict(bases=good["proofs"]),
           dict(scalars=good["keys"]), dict(status=good["index"]), dict(where=good["off"] + 1), dict(n=(1 << 31) // ROWS + 1, stride=1 << 40)]
    for change in bad:
        assert call(**change) == 2, change
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((big == SENT).all())
    # ... and the same arguments unchanged do write all four
    assert call() == 0
    torch.cuda.synchronize()
    h = corpus[4]
    assert bytes(status.cpu().numpy()) == h[2][:n] and bases.cpu().numpy().tobytes() == h[0][:96 * ROWS * n]
    assert bool((big[160 * ROWS * n + 16 + n:] == SENT).all()) and bool((big[160 * ROWS * n + n:160 * ROWS * n + 16] == SENT).all())
