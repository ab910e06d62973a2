"""GPU: proofs of circuits with range_gate items -- the range widget's term in the quotient, in r(X) and in
the verifier's sides.  Two circuits of mixed appends plus range items of 8, 16 and 62 bits: one padded to 2^7 with spare rows, one
of exactly 2^6 rows; each unblinded and blinded.  A proof is accepted by Proof.verify, verify_batch, verify_each and the trapdoor
model of tests/plonk_verify_range_model.py iff every witness is in range; rejected with a_next_eval changed, with the key's q_range
commitment swapped for another circuit's, and under the key of the same circuit built with num_bits + 2; verify_encoded refuses
such keys; a circuit without range items proves to the bytes it proves to with no eighteenth input anywhere; and after
clear_witness the same calls find their rows in place and the proof verifies and is deterministic."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonk_verify_model as V  # noqa: E402
import plonk_verify_range_model as VR  # noqa: E402

R = V.R
S = pg.BlsScalar.from_int
TAU = 0x5EED_7A2 ** 9 % R
SIZES = {"spare_rows": 1 << 7, "no_spare_rows": 1 << 6}
BITS = (8, 16, 62)
GOOD = {8: [200, 255, 0], 16: [65535, 12345], 62: [2**62 - 1, 2**61 + 5]}
BLINDERS = [random.Random(77).randrange(R) for _ in range(11)]


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def tv(xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.int64, device="cuda")


def dev_scalars(vals):
    return torch.from_numpy(synth.scalars_from_ints(vals).view(np.int64)).cuda()


def build(engine, kind, values=GOOD, extra_bits=0, comp=None):
    """mixed appends (a ladder range_check, scalar gadgets, a public input, batched gates), then range items of 8, 16 and 62 bits
    (+ extra_bits on the 8-bit ones): single calls and batches, on Variables of add_input, add_input_batch and mul_batch"""
    comp = comp or pg.StandardComposer(engine, 1 << 10, 1 << 10)
    a, b = pg.AllocatedScalar.allocate(comp, S(100)), pg.AllocatedScalar.allocate(comp, S(100))
    if kind == "spare_rows":
        res = pg.range_check(comp, S(3), S(200), a)
        comp.constrain_to_constant(res, S(1), None)
        comp.constrain_to_constant(pg.maybe_equal(comp, a, b), S(1), None)
    else:
        comp.constrain_to_constant(pg.conditionally_select_zero(comp, b.var, comp.add_input(S(1))), S(100), None)
    comp.constrain_to_constant(comp.add_input(S(9)), S(20), S(11))  # 9 - 20 + PI(11) = 0: one public input
    one = comp.add_input(S(1))
    first = comp.add_input_batch(dev_scalars(values[8]))
    w8 = comp.mul_batch(S(1), tv(range(first, first + len(values[8]))), tv([one] * len(values[8])), S(0))  # copies: results of a mul
    comp.range_gate_batch(w8, 8 + extra_bits)
    first = comp.add_input_batch(dev_scalars(values[16]))
    comp.range_gate_batch(tv(range(first, first + len(values[16]))), 16)
    for v in values[62]:
        comp.range_gate(comp.add_input(S(v)), 62)
    comp.sync()
    if kind == "no_spare_rows":
        x = comp.add_input(S(3))
        assert comp.circuit_size() <= SIZES[kind] - 2
        while comp.circuit_size() + 2 <= SIZES[kind]:
            comp.range_gate(x, 2)
        while comp.circuit_size() < SIZES[kind]:
            comp.constrain_to_constant(x, S(3), None)
        comp.sync()
        assert comp.circuit_size() == SIZES[kind]
    assert 1 << (comp.circuit_size() - 1).bit_length() == SIZES[kind], comp.circuit_size()
    return comp


def public_inputs(comp) -> dict:
    dense = comp.construct_dense_pi_vec().cpu().numpy().view(np.uint64)
    return {i: synth.to_int(row) for i, row in enumerate(dense.tolist()) if any(row)}


@pytest.fixture(scope="module")
def keys(engine):
    ck = pg.CommitKey.setup(engine, (1 << 7) + 7, S(TAU))
    ok = pg.OpeningKey.setup(engine, S(TAU))
    yield ck, ok
    ok.close()


@pytest.fixture(scope="module", params=list(SIZES))
def world(engine, keys, request):
    ck, ok = keys
    comp = build(engine, request.param)
    assert comp.check() == -1 and comp.copy_constraints_hold()
    n = SIZES[request.param]
    pre = comp.preprocessed_commitments(ck)
    assert not pre["q_range"].is_identity()
    yield request.param, comp, ck, ok, pg.VerifierKey(n, pre), pre, public_inputs(comp), n
    comp.close()


def all_verifiers(proof, vk, pre, ok, pi, n) -> set:
    """the verdicts of Proof.verify, verify_batch, verify_each and the trapdoor model (one element when they agree)"""
    return {proof.verify(vk, ok, pi), pg.verify_batch([proof], vk, ok, pi), pg.verify_each([proof], vk, ok, pi)[0],
            VR.verify(proof, pre, pi, n, TAU)}


@pytest.mark.parametrize("blinding", [None, True])
def test_a_satisfied_circuit_verifies_and_tampering_is_rejected(world, blinding):
    kind, comp, ck, ok, vk, pre, pi, n = world
    proof = comp.prove(ck, b"plonk", pre, blinding=blinding)
    assert len(proof.to_bytes()) == 1040
    assert all_verifiers(proof, vk, pre, ok, pi, n) == {True}
    # the parent's verifier algebra (no range term) does not accept it
    assert not V.verify(proof, pre, pi, n, TAU)
    # a_next_eval changed: the second opening and rho_range both see it
    bad = pg.Proof.from_bytes(proof.to_bytes())
    bad.a_next_eval = S((proof.a_next_eval.to_int() + 1) % R)
    assert all_verifiers(bad, vk, pre, ok, pi, n) == {False}
    # the key's q_range commitment swapped for another circuit's (the other size's: other rows carry the widget)
    other = build(comp.engine, "no_spare_rows" if kind == "spare_rows" else "spare_rows")
    swapped = dict(pre, q_range=other.preprocessed_commitments(ck)["q_range"])
    other.close()
    assert swapped["q_range"] != pre["q_range"]
    assert all_verifiers(proof, pg.VerifierKey(n, swapped), swapped, ok, pi, n) == {False}
    # the key of the same circuit built with num_bits + 2 on its 8-bit items (the same witnesses satisfy it too)
    wider = build(comp.engine, kind, extra_bits=2)
    assert wider.check() == -1 and wider.circuit_size() <= n
    pre_w = wider.preprocessed_commitments(ck, n)
    wider.close()
    assert all_verifiers(proof, pg.VerifierKey(n, pre_w), pre_w, ok, pi, n) == {False}
    # pg_plonk_sides has no row for the term
    with pytest.raises(ValueError, match="q_range"):
        pg.verify_encoded(proof.to_bytes(), vk, ok, pi)
    # another public input
    assert not proof.verify(vk, ok, {row: (v + 1) % R for row, v in pi.items()})


@pytest.mark.parametrize("blinding", [None, True])
@pytest.mark.parametrize("bits", BITS)
def test_a_witness_out_of_range_is_rejected(engine, keys, world, blinding, bits):
    kind, _, ck, ok, vk, pre, pi, n = world
    values = {b: list(v) for b, v in GOOD.items()}
    values[bits][-1] = 2**bits if bits != 16 else R - 1
    comp = build(engine, kind, values)
    assert comp.check() >= 3 and comp.copy_constraints_hold()
    assert comp.preprocessed_commitments(ck) == pre  # the same circuit: the verifier's key is the honest one
    proof = comp.prove(ck, b"plonk", pre, blinding=blinding)
    comp.close()
    assert all_verifiers(proof, vk, pre, ok, pi, n) == {False}


@pytest.mark.parametrize("blinding", [None, BLINDERS])
def test_a_circuit_without_range_items_proves_as_before(engine, keys, blinding, monkeypatch):
    """no q_range among the prover's inputs, pg_quotient_range never called, the key's q_range the identity, the sides those of
    a key without the widget (verify_encoded accepts it) -- and the bytes those of a prover that cannot pass the input at all"""
    ck, ok = keys
    comp = pg.StandardComposer(engine, 1 << 10, 1 << 10)
    a = pg.AllocatedScalar.allocate(comp, S(100))
    comp.constrain_to_constant(pg.range_check(comp, S(3), S(200), a), S(1), None)
    comp.constrain_to_constant(comp.add_input(S(9)), S(20), S(11))
    pre = comp.preprocessed_commitments(ck)
    assert pre["q_range"].is_identity()
    n = 1 << (comp.circuit_size() - 1).bit_length()
    assert "q_range" not in comp.prover_polynomials(S(1), S(2))
    proof = comp.prove(ck, b"plonk", pre, blinding=blinding)
    eng = comp.engine
    plain_q, plain_qb = eng.quotient, eng.quotient_blinded

    def without(fn):
        def call(*args, q_range=None, **kw):
            assert q_range is None
            return fn(*args, **kw)
        return call
    monkeypatch.setattr(eng, "quotient", without(plain_q))
    monkeypatch.setattr(eng, "quotient_blinded", without(plain_qb))
    monkeypatch.setattr(eng._lib, "pg_quotient_range", None)
    assert comp.prove(ck, b"plonk", pre, blinding=blinding).to_bytes() == proof.to_bytes()
    monkeypatch.undo()
    vk, pi = pg.VerifierKey(n, pre), public_inputs(comp)
    assert proof.verify(vk, ok, pi) and V.verify(proof, pre, pi, n, TAU) and VR.verify(proof, pre, pi, n, TAU)
    assert pg.verify_encoded(proof.to_bytes(), vk, ok, pi) == [True]
    comp.close()


def test_clear_witness_refreshes_in_place_and_the_proof_is_deterministic(engine, keys, world):
    kind, _, ck, ok, vk, pre, pi, n = world
    comp = build(engine, kind)
    rows = comp.circuit_size()
    comp.clear_witness()
    second = {8: [1, 2, 3], 16: [0, 65535], 62: [5, 2**62 - 1]}
    build(engine, kind, second, comp=comp)
    kept, rewritten, refreshing = comp.refresh_stats()
    assert (kept, rewritten, refreshing) == (rows - 3, 0, True)
    assert comp.check() == -1
    assert comp.preprocessed_commitments(ck) == pre
    proof = comp.prove(ck, b"plonk", pre, blinding=BLINDERS)
    assert all_verifiers(proof, vk, pre, ok, pi, n) == {True}
    assert comp.prove(ck, b"plonk", pre, blinding=BLINDERS).to_bytes() == proof.to_bytes()
    fresh = build(engine, kind, second)
    assert fresh.prove(ck, b"plonk", pre, blinding=BLINDERS).to_bytes() == proof.to_bytes()
    fresh.close()
    # a third set with a witness out of range: still in place, and rejected
    comp.clear_witness()
    build(engine, kind, {**second, 62: [2**62, 1]}, comp=comp)
    assert comp.refresh_stats() == (rows - 3, 0, True) and comp.check() >= 3
    assert all_verifiers(comp.prove(ck, b"plonk", pre), vk, pre, ok, pi, n) == {False}
    comp.close()
