"""GPU: proofs of a circuit with is_less_equal items.  Nothing in the prover or the verifier is new -- the
widget rows are range_gate's and the terminal row is an arithmetic row -- so this checks the composition end to end: x and y bounded
by range_gate_batch at 64 bits (the gadget's precondition), is_less_equal_each, the bits as selects of a
conditionally_select_zero_batch, and two of the bits constrained to constants.  A proof, blinded and not, is accepted by Proof.verify,
verify_each, verify_batch and verify_encoded(range_term=True); rejected when a witness changes so that a constrained bit flips;
rejected under the key of the same circuit with `strict` flipped (which the same witnesses satisfy); and a circuit without compare
items proves to the bytes recorded before the gadget existed (tests/golden/prove_without_interval.json)."""
import json

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
import test_gpu_prove_interval as tpi
from plonk_gadgets_amd import synth

pytestmark = pytest.mark.gpu

R = tpi.R
S = pg.BlsScalar.from_int
TAU = tpi.TAU
NUM_BITS = 64
# x < y, x = y, x > y; the bits of items 0 and 2 are constrained (1 and 0 under either `strict`), item 1's is 1 or 0 by `strict`
GOOD = [(5, 2**64 - 1), (2**63 + 9, 2**63 + 9), (2**64 - 1, 2**64 - 2)]


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def tv(xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.int64, device="cuda")


def build(engine, values=GOOD, strict=False):
    comp = pg.StandardComposer(engine, 1 << 10, 1 << 10)
    comp.constrain_to_constant(comp.add_input(S(9)), S(20), S(11))  # 9 - 20 + PI(11) = 0: one public input
    n = len(values)
    first = comp.add_input_batch(tpi.dev_scalars([x for x, _ in values] + [y for _, y in values]))
    xs, ys = tv(range(first, first + n)), tv(range(first + n, first + 2 * n))
    comp.range_gate_batch(xs, NUM_BITS)
    comp.range_gate_batch(ys, NUM_BITS)
    bits = comp.is_less_equal_each(xs, ys, NUM_BITS, strict)
    comp.conditionally_select_zero_batch(xs, bits)      # x if the bit is 1, else 0
    comp.constrain_to_constant_batch(bits[:1], S(1))
    comp.constrain_to_constant_batch(bits[2:], S(0))
    comp.sync()
    return comp, bits.cpu().tolist()


@pytest.fixture(scope="module")
def keys(engine):
    ck = pg.CommitKey.setup(engine, (1 << 8) + 7, S(TAU))
    ok = pg.OpeningKey.setup(engine, S(TAU))
    yield ck, ok
    ok.close()


@pytest.fixture(scope="module")
def world(engine, keys):
    ck, ok = keys
    comp, bits = build(engine)
    assert comp.check() == -1 and comp.copy_constraints_hold()
    n = 1 << (comp.circuit_size() - 1).bit_length()
    pre = comp.preprocessed_commitments(ck)
    assert not pre["q_range"].is_identity()
    yield comp, ck, ok, pg.VerifierKey(n, pre), pre, tpi.public_inputs(comp), n
    comp.close()


def all_verifiers(proof, vk, ok, pi) -> set:
    """the verdicts of Proof.verify, verify_batch, verify_each and verify_encoded with the range row (one element when they agree)"""
    return {proof.verify(vk, ok, pi), pg.verify_batch([proof], vk, ok, pi), pg.verify_each([proof], vk, ok, pi)[0],
            pg.verify_encoded(proof.to_bytes(), vk, ok, pi, range_term=True)[0]}


@pytest.mark.parametrize("blinding", [None, True])
def test_a_satisfied_circuit_verifies_and_the_other_strictness_is_rejected(world, blinding):
    comp, ck, ok, vk, pre, pi, n = world
    proof = comp.prove(ck, b"plonk", pre, blinding=blinding)
    assert all_verifiers(proof, vk, ok, pi) == {True}
    # the key of the same circuit with `strict` flipped: the same witnesses satisfy it, its q_c column differs
    other, _ = build(comp.engine, strict=True)
    assert other.check() == -1 and other.circuit_size() == comp.circuit_size()
    pre_s = other.preprocessed_commitments(ck, n)
    assert pre_s["q_c"] != pre["q_c"] and pre_s["q_range"] == pre["q_range"] and pre_s["q_l"] == pre["q_l"]
    assert all_verifiers(proof, pg.VerifierKey(n, pre_s), ok, pi) == {False}
    # ... and that circuit's own proof is accepted under its key, rejected under this one
    proof_s = other.prove(ck, b"plonk", pre_s, blinding=blinding)
    other.close()
    assert all_verifiers(proof_s, pg.VerifierKey(n, pre_s), ok, pi) == {True}
    assert all_verifiers(proof_s, vk, ok, pi) == {False}


@pytest.mark.parametrize("blinding", [None, True])
@pytest.mark.parametrize("item", (0, 2))
def test_a_witness_that_flips_a_constrained_bit_is_rejected(engine, world, blinding, item):
    _, ck, ok, vk, pre, pi, n = world
    values = list(GOOD)
    x, y = values[item]
    values[item] = (y, x)       # still below 2^64: every widget holds, the bit is the other one, the constant's row fails
    comp, bits = build(engine, values)
    bad = comp.check()
    assert bad >= comp.circuit_size() - 2 and comp.copy_constraints_hold()
    assert comp.preprocessed_commitments(ck) == pre  # the same circuit: the verifier's key is the honest one
    proof = comp.prove(ck, b"plonk", pre, blinding=blinding)
    comp.close()
    assert all_verifiers(proof, vk, ok, pi) == {False}


def test_the_bits_are_the_comparisons(engine):
    for strict in (False, True):
        comp, bits = build(engine, strict=strict)
        vals = np.ascontiguousarray(np.asarray(comp.export()["var_values"])).view(np.uint64).reshape(-1, 4)
        got = [synth.to_int(vals[b]) for b in bits]
        assert got == [int(x < y if strict else x <= y) for x, y in GOOD]
        comp.close()


@pytest.mark.parametrize("blinding", ["unblinded", "fixed_blinders"])
def test_a_circuit_without_compare_items_proves_to_the_recorded_bytes(engine, keys, blinding):
    """the golden file holds the two proofs as a commit before the gadget produced them (same circuit, trapdoor and blinders)"""
    ck, ok = keys
    with open(tpi.GOLDEN) as f:
        golden = json.load(f)
    assert golden["blinders"] == [hex(b) for b in tpi.BLINDERS] and golden["tau"] == hex(TAU)
    comp = tpi.circuit_without_interval_items(engine)
    pre = comp.preprocessed_commitments(ck)
    proof = comp.prove(ck, b"plonk", pre, blinding=None if blinding == "unblinded" else tpi.BLINDERS)
    assert proof.to_bytes().hex() == golden[blinding]
    n = 1 << (comp.circuit_size() - 1).bit_length()
    assert proof.verify(pg.VerifierKey(n, pre), ok, tpi.public_inputs(comp))
    comp.close()
