"""GPU: verify_encoded -- the verifier's sides built on the device from proof bytes -- says what verify says, proof by proof.

The three circuits and the cases of tests/test_gpu_verify_each_segmented.py, built the same way (a range check, constant gates with
a public input, both; honest, a spoiled evaluation, two and three coinciding commitments), and the off-curve case in bytes: a
commitment whose x has no y, and one that is a curve point outside G1.  Batches of 1, 2, 17 and 65 with mixed keys and public
inputs; exactly one pg_plonk_sides, one pg_msm_segmented, one pg_pairing_check and no pg_msm per call; bytes, tensors and Proof
objects give the same answer; a batch rejected entirely before the pairing is all False.  And real proofs under four labels that
put the end of the sponge's first block after the seed on bytes the label b"plonk" never puts it on."""
import pytest
import torch

import plonk_gadgets_amd as pg
import plonk_sides_corpus as K
import strobe_model as sm
from plonk_gadgets_amd import verifier as V

pytestmark = pytest.mark.gpu

S = pg.BlsScalar.from_int
TAU = 0x5EED_7A0 ** 9


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def circuit(engine, ck, kind, label=b"plonk"):
    comp = pg.StandardComposer(engine, 1 << 12, 1 << 12)
    pi = {}
    if kind != 1:  # a range check: the ladder's selectors
        res = pg.range_check(comp, S(50_000), S(250_000), pg.AllocatedScalar.allocate(comp, S(60_000 + kind)))
        comp.constrain_to_constant(res, S(1), None)
    if kind != 0:  # plain constant gates, the last with a public input
        for t in range(3):
            comp.constrain_to_constant(comp.add_input(S(t + 2)), S(t + 2), None)
        comp.constrain_to_constant(comp.add_input(S(9)), S(20), S(11))  # 9 - 20 + PI = 0
    comp.sync()
    assert comp.check() == -1
    if kind != 0:
        import numpy as np
        from plonk_gadgets_amd import synth
        dense = comp.construct_dense_pi_vec().cpu().numpy().view(np.uint64)
        pi = {i: synth.to_int(row) for i, row in enumerate(dense.tolist()) if any(row)}
        assert pi
    pre = comp.preprocessed_commitments(ck)
    n = 1 << max(0, (comp.circuit_size() - 1).bit_length())
    out = (comp.prove(ck, label, pre), pg.VerifierKey(n, pre), pi)
    comp.close()
    return out


@pytest.fixture(scope="module")
def setup(engine):
    ck = pg.CommitKey.setup(engine, (1 << 12) - 1, S(TAU))
    ok = pg.OpeningKey.setup(engine, S(TAU))
    yield ck, ok
    ok.close()


@pytest.fixture(scope="module")
def world(engine, setup):
    """[(proof bytes, key, public inputs)], what verify says of each (False where the bytes are no Proof), the status
    verify_encoded must give, the opening key"""
    ck, ok = setup
    three = [circuit(engine, ck, kind) for kind in range(3)]
    cases = [(p.to_bytes(), vk, pi) for p, vk, pi in three]
    spoiled = pg.Proof.from_bytes(cases[1][0])
    spoiled.c_eval = spoiled.c_eval + S(1)
    cases.append((spoiled.to_bytes(), three[1][1], three[1][2]))
    for fields in (("c_comm",), ("c_comm", "a_comm")):  # commitments that coincide
        m = pg.Proof.from_bytes(cases[0][0])
        for f in fields:
            setattr(m, f, m.b_comm)
        cases.append((m.to_bytes(), three[0][1], three[0][2]))
    enc = K.rejected_encodings()
    cases.append((K.with_commitment(cases[2][0], 0, enc["x-with-no-y"][0]), three[2][1], three[2][2]))
    cases.append((K.with_commitment(cases[2][0], 4, enc["outside-the-subgroup"][0]), three[2][1], three[2][2]))
    cases.append((cases[1][0], three[1][1], None))  # an honest proof without its public input
    verdicts = []
    for data, vk, pi in cases:
        try:
            verdicts.append(pg.verify(pg.Proof.from_bytes(data), vk, ok, pi))
        except ValueError:
            verdicts.append(False)
    assert verdicts == [True, True, True, False, False, False, False, False, False]
    status = [(0, 0)] * 6 + [(2, 0), (3, 4), (0, 0)]
    return cases, verdicts, status, ok


@pytest.fixture
def counted(monkeypatch, engine):
    calls = {"pg_msm": 0, "pg_msm_segmented": 0, "pg_plonk_sides": 0, "pg_pairing_check": 0}
    for name in calls:
        real = getattr(engine._lib, name)

        def wrapper(*args, _real=real, _name=name):
            calls[_name] += 1
            return _real(*args)
        monkeypatch.setattr(engine._lib, name, wrapper)
    return calls


@pytest.mark.parametrize("picks", [[0], [3], [6], [1, 7], [(5 * i) % 9 for i in range(17)], [(4 * i + i // 9) % 9 for i in range(65)]],
                         ids=["1", "1-spoiled", "1-no-y", "2-outside-G1", "17", "65"])
def test_verify_encoded_is_verify_proof_by_proof(engine, world, counted, picks):
    cases, verdicts, status, ok = world
    data = b"".join(cases[k][0] for k in picks)
    vks, pis = [cases[k][1] for k in picks], [cases[k][2] for k in picks]
    got, st, wh = pg.verify_encoded(data, vks, ok, pis, return_status=True)
    assert counted == {"pg_msm": 0, "pg_msm_segmented": 1, "pg_plonk_sides": 1, "pg_pairing_check": 1}, counted
    assert got == [verdicts[k] for k in picks]
    assert list(zip(st, wh)) == [status[k] for k in picks]
    if len(picks) >= 17:
        assert len({id(v) for v in vks}) == 3 and True in got and False in got


def test_bytes_tensors_and_proofs_give_the_same_answer(engine, world):
    cases, verdicts, _, ok = world
    picks = [0, 1, 3, 2, 4, 8]
    data = b"".join(cases[k][0] for k in picks)
    vks, pis = [cases[k][1] for k in picks], [cases[k][2] for k in picks]
    want = [verdicts[k] for k in picks]
    host = torch.frombuffer(bytearray(data), dtype=torch.uint8).view(len(picks), V.PROOF_BYTES)
    assert pg.verify_encoded(data, vks, ok, pis) == want
    assert pg.verify_encoded(bytearray(data), vks, ok, pis) == want
    assert pg.verify_encoded(host, vks, ok, pis) == want
    assert pg.verify_encoded(host.to(engine.device), vks, ok, pis) == want
    assert pg.verify_encoded([pg.Proof.from_bytes(cases[k][0]) for k in picks], vks, ok, pis) == want
    # one key, one label, one set of public inputs for all
    assert pg.verify_encoded(cases[1][0] * 3, cases[1][1], ok, cases[1][2]) == [True] * 3
    assert pg.verify_encoded(cases[1][0] * 3, cases[1][1], ok, cases[1][2], label=b"another") == [False] * 3
    assert pg.verify_encoded(b"", vks, ok) == [] and pg.verify_encoded([], vks, ok, return_status=True) == ([], [], [])
    with pytest.raises(ValueError):
        pg.verify_encoded(data[:-1], vks, ok, pis)


def test_a_batch_rejected_before_the_pairing_is_all_false(engine, world, counted):
    cases, _, status, ok = world
    bad_eval = K.with_evaluation(cases[0][0], 5, K.R)
    data = cases[6][0] + cases[7][0] + bad_eval + cases[6][0]
    got, st, wh = pg.verify_encoded(data, [cases[6][1], cases[7][1], cases[0][1], cases[6][1]], ok,
                                    [cases[6][2], cases[7][2], None, {1 << 12: 1}], return_status=True)
    assert got == [False] * 4 and list(zip(st, wh)) == [(2, 0), (3, 4), (5, 5), (2, 0)]
    assert counted["pg_plonk_sides"] == 1 and counted["pg_msm"] == 0


# what ends the first block after the key's seed (strobe_model.sides_phase0_classes) -> a label that puts it there
BOUNDARY_LABELS = {"begin-first": b"plnk", "commitment-first": b"pk", "commitment-last": b"plonk-verifier", "length-0": b"plonk-v2"}


def test_real_proofs_under_labels_that_end_a_block_where_the_others_do_not(engine, setup):
    """the four labels of tests/plonk_sides_corpus.py end that block inside a message, on the last length byte or on a flags byte;
    these four end it on begin_op's first framing byte, on the first and on the last byte of a commitment, and on the first byte
    of a length word.  A proof verifies under its own label alone, and verify_encoded says what verify says."""
    ck, ok = setup
    labels = list(BOUNDARY_LABELS.values())
    proved = [circuit(engine, ck, 2, lab) for lab in labels]
    vk, pi = proved[0][1], proved[0][2]
    assert all(v == vk and q == pi for _, v, q in proved)
    old = set().union(*(sm.sides_phase0_classes(lab, vk.n) for lab in K.LABELS))  # (n travels as 8 bytes whatever it is)
    for cls, lab in BOUNDARY_LABELS.items():
        assert cls in sm.sides_phase0_classes(lab, vk.n) and cls not in old, cls
    assert len({vk.record(ok, lab)[200] for lab in labels}) == 4  # four seed positions
    pairs = [(i, j) for i in range(4) for j in range(4)]
    data = b"".join(proved[i][0].to_bytes() for i, _ in pairs)
    got, st, _ = pg.verify_encoded(data, vk, ok, pi, label=[labels[j] for _, j in pairs], return_status=True)
    assert got == [i == j for i, j in pairs] and st == [0] * 16
    assert [pg.verify(proved[i][0], vk, ok, pi, labels[j]) for i, j in pairs] == got
