"""GPU: verify_encoded(..., range_term=True) on real proofs of circuits with range_gate items (n = 2^6) and
with interval_gate items (n = 2^7), unblinded and blinded: it says what Proof.verify says, proof by proof -- for the honest proof,
a_next_eval + 1, the key's q_range swapped for another circuit's, the key of the same circuit with num_bits + 2, a proof made
with a witness out of range (out of its interval), and a call that holds a range-circuit proof and a plain-circuit proof under
their own keys.  The same honest proof through the 23-row table and the same MSM and pairing check is rejected: row 23 is what
makes it pass.  Without the flag such a key is still refused, and for a circuit without range items the flag changes no verdict.
The circuits are those of tests/test_gpu_prove_range.py and tests/test_gpu_prove_interval.py."""
import pytest
import torch

import plonk_gadgets_amd as pg
import plonk_sides_corpus as K
import test_gpu_prove_interval as PI
import test_gpu_prove_range as PR
from plonk_gadgets_amd.verifier import RANGE_SIDES_ROWS, SIDES_ROWS, pairing_check

pytestmark = pytest.mark.gpu

R, S, TAU = PR.R, PR.S, PR.TAU
BLINDINGS = {"unblinded": None, "blinded": True}
CIRCUITS = ("range", "interval")


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(engine):
    ck = pg.CommitKey.setup(engine, (1 << 7) + 7, S(TAU))
    ok = pg.OpeningKey.setup(engine, S(TAU))
    yield ck, ok
    ok.close()


def wider_interval_circuit(engine):
    """tests/test_gpu_prove_interval.py's circuit with num_bits + 2 on its 8-bit items"""
    comp = pg.StandardComposer(engine, 1 << 10, 1 << 10)
    batch = comp.interval_gate_batch
    comp.interval_gate_batch = lambda w, lo, hi, bits: batch(w, lo, hi, bits + 2)
    PI.build(engine, "spare_rows", comp=comp)
    del comp.interval_gate_batch
    return comp


def make_world(engine, ck, which):
    """the circuit, its key and public inputs, an honest proof and a proof with one witness out of bounds per blinding, and the
    two foreign keys: q_range swapped for another circuit's, and the same circuit with num_bits + 2 on its 8-bit items"""
    if which == "range":
        mod, kind, other_kind = PR, "no_spare_rows", "spare_rows"
        bad_values = {b: list(v) for b, v in PR.GOOD.items()}
        bad_values[62][-1] = 2**62
        wider = PR.build(engine, kind, extra_bits=2)
    else:
        mod, kind, other_kind = PI, "spare_rows", "no_spare_rows"
        bad_values = {b: list(v) for b, v in PI.GOOD.items()}
        bad_values[8][-1] = 301
        wider = wider_interval_circuit(engine)
    n = mod.SIZES[kind]
    comp = mod.build(engine, kind)
    assert comp.check() == -1
    pre = comp.preprocessed_commitments(ck)
    assert not pre["q_range"].is_identity() and 1 << 6 <= n <= 1 << 8
    pi = mod.public_inputs(comp)
    honest = {name: comp.prove(ck, b"plonk", pre, blinding=b) for name, b in BLINDINGS.items()}
    comp.close()
    bad = mod.build(engine, kind, bad_values)
    assert bad.check() >= 3 and bad.preprocessed_commitments(ck) == pre
    out_of_bounds = {name: bad.prove(ck, b"plonk", pre, blinding=b) for name, b in BLINDINGS.items()}
    bad.close()
    other = mod.build(engine, other_kind)
    swapped = dict(pre, q_range=other.preprocessed_commitments(ck)["q_range"])
    other.close()
    assert swapped["q_range"] != pre["q_range"]
    assert wider.check() == -1 and wider.circuit_size() <= n
    pre_w = wider.preprocessed_commitments(ck, n)
    wider.close()
    assert pre_w != pre  # (10 bits take the rows of 8: q_range may be the same commitment, the other selectors are not)
    return {"n": n, "vk": pg.VerifierKey(n, pre), "pi": pi, "honest": honest, "out_of_bounds": out_of_bounds,
            "vk_swapped": pg.VerifierKey(n, swapped), "vk_wider": pg.VerifierKey(n, pre_w)}


@pytest.fixture(scope="module")
def worlds(engine, keys):
    """which -> make_world(which), each built once, when a test first asks for it"""
    class Worlds(dict):
        def __missing__(self, which):
            self[which] = make_world(engine, keys[0], which)
            return self[which]
    return Worlds()


@pytest.fixture(scope="module")
def plain(engine, keys):
    """a circuit without range items: its key's q_range is the identity"""
    ck, _ = keys
    comp = pg.StandardComposer(engine, 1 << 10, 1 << 10)
    a = pg.AllocatedScalar.allocate(comp, S(100))
    comp.constrain_to_constant(pg.range_check(comp, S(3), S(200), a), S(1), None)
    comp.constrain_to_constant(comp.add_input(S(9)), S(20), S(11))
    pre = comp.preprocessed_commitments(ck)
    assert pre["q_range"].is_identity()
    n = 1 << (comp.circuit_size() - 1).bit_length()
    out = {"vk": pg.VerifierKey(n, pre), "pi": PR.public_inputs(comp), "honest": comp.prove(ck, b"plonk", pre, blinding=True)}
    comp.close()
    return out


def tampered(proof):
    bad = pg.Proof.from_bytes(proof.to_bytes())
    bad.a_next_eval = S((proof.a_next_eval.to_int() + 1) % R)
    return bad


@pytest.mark.parametrize("blinding", list(BLINDINGS))
@pytest.mark.parametrize("which", CIRCUITS)
def test_the_verdicts_are_proof_verifys(worlds, keys, which, blinding):
    """the five cases in ONE call of verify_encoded: five proofs under three keys"""
    ok = keys[1]
    w = worlds[which]
    honest = w["honest"][blinding]
    cases = [("honest", honest, w["vk"], True), ("a_next_eval + 1", tampered(honest), w["vk"], False),
             ("q_range swapped", honest, w["vk_swapped"], False), ("num_bits + 2", honest, w["vk_wider"], False),
             ("a witness out of bounds", w["out_of_bounds"][blinding], w["vk"], False)]
    want = [p.verify(vk, ok, w["pi"]) for _, p, vk, _ in cases]
    assert want == [expected for _, _, _, expected in cases]
    got, status, where = pg.verify_encoded([p for _, p, _, _ in cases], [vk for _, _, vk, _ in cases], ok, w["pi"], return_status=True,
                                           range_term=True)
    assert got == want and status == [0] * 5 and where == [0] * 5  # (every rejection here is the pairing check's)
    # ... and one at a time, as bytes
    assert pg.verify_encoded(honest.to_bytes(), w["vk"], ok, w["pi"], range_term=True) == [True]
    assert pg.verify_encoded(tampered(honest).to_bytes(), w["vk"], ok, w["pi"], range_term=True) == [False]


def test_a_range_proof_and_a_plain_proof_in_one_call(worlds, plain, keys):
    ok = keys[1]
    proofs, vks, pis = [], [], []
    for which in CIRCUITS:
        w = worlds[which]
        proofs += [w["honest"]["blinded"], plain["honest"], tampered(w["honest"]["unblinded"]), tampered(plain["honest"])]
        vks += [w["vk"], plain["vk"], w["vk"], plain["vk"]]
        pis += [w["pi"], plain["pi"], w["pi"], plain["pi"]]
    want = [p.verify(vk, ok, pi) for p, vk, pi in zip(proofs, vks, pis)]
    assert want == [True, True, False, False] * 2
    assert pg.verify_encoded(proofs, vks, ok, pis, range_term=True) == want
    # a proof under the other proof's key is rejected, whichever way round
    assert pg.verify_encoded(proofs[:2], [vks[1], vks[0]], ok, pis[:2], range_term=True) == [False, False]


def table_verdict(engine, ok, proof, vk, pi, range_term):
    """Engine.plonk_sides, the segmented MSM over the uniform offsets and the pairing check, as verify_encoded chains them"""
    rows = RANGE_SIDES_ROWS if range_term else SIDES_ROWS
    dev = engine.device
    off, pi_rows, vals = K.csr([pi])
    d = lambda raw: torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    signed = [w - (1 << 64) if w >> 63 else w for w in vals]
    bases, scalars, status, _ = engine.plonk_sides(
        d(proof.to_bytes()), d(vk.record(ok, b"plonk", range_term)), None, torch.tensor(off, dtype=torch.int64, device=dev),
        torch.tensor(pi_rows, dtype=torch.int64, device=dev), torch.tensor(signed, dtype=torch.int64, device=dev).view(-1, 4),
        range_term=range_term)
    assert bases.shape[0] == rows and status.cpu().tolist() == [0]
    sums = engine.msm_segmented(bases, scalars, [0, rows])
    return bool(pairing_check(engine, sums, [ok.prepared_tau_h, ok.prepared_h]).cpu().tolist()[0])


@pytest.mark.parametrize("which", CIRCUITS)
def test_the_23_row_table_rejects_what_the_24_row_table_accepts(engine, worlds, keys, which):
    ok = keys[1]
    w = worlds[which]
    proof = w["honest"]["blinded"]
    assert proof.verify(w["vk"], ok, w["pi"])
    assert table_verdict(engine, ok, proof, w["vk"], w["pi"], range_term=True)
    assert not table_verdict(engine, ok, proof, w["vk"], w["pi"], range_term=False)
    # without the flag verify_encoded still refuses the key
    with pytest.raises(ValueError, match="q_range"):
        pg.verify_encoded(proof.to_bytes(), w["vk"], ok, w["pi"])
    with pytest.raises(ValueError, match="q_range"):
        pg.verify_encoded(proof.to_bytes(), w["vk"], ok, w["pi"], range_term=False)


def test_a_circuit_without_range_items_gets_the_same_verdicts_either_way(plain, keys):
    ok = keys[1]
    proofs = [plain["honest"], tampered(plain["honest"]), plain["honest"]]
    pis = [plain["pi"], plain["pi"], {row: (v + 1) % R for row, v in plain["pi"].items()}]
    want = [p.verify(plain["vk"], ok, pi) for p, pi in zip(proofs, pis)]
    assert want == [True, False, False]
    with_flag = pg.verify_encoded(proofs, plain["vk"], ok, pis, return_status=True, range_term=True)
    without = pg.verify_encoded(proofs, plain["vk"], ok, pis, return_status=True)
    assert with_flag == without and with_flag[0] == want
    assert pg.verify_encoded([], plain["vk"], ok, range_term=True) == []
