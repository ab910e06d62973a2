"""GPU: proofs of circuits with interval_gate items.  Nothing in the prover or the verifier is new -- the
widget rows are range_gate's and the terminal rows are arithmetic rows -- so this checks the composition end to end.  Two circuits
of mixed appends plus interval items of 8 bits (one pair for the batch, on results of a mul_batch), 16 bits (a pair per item) and
62 bits (single calls): one padded to 2^7 with spare rows, one of exactly 2^6 rows; each unblinded and blinded.  A proof is accepted
by Proof.verify, verify_batch, verify_each and the trapdoor model of tests/plonk_verify_range_model.py iff every witness lies in
its interval; rejected under the key of the same circuit built with one bound moved by one (which the same witnesses satisfy);
deterministic after clear_witness; and a circuit without interval items proves to the bytes recorded before the gadget existed
(tests/golden/prove_without_interval.json)."""
import json
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
# bits -> (lo, hi) per item; the 8-bit pair is the batch's one pair
BOUNDS = {8: [(100, 300)] * 2, 16: [(0, 65535), (R - 1 - 40000, R - 1)], 62: [(5, 5 + 2**62 - 1)]}
GOOD = {8: [100, 300], 16: [65535, R - 1], 62: [2**61]}
BLINDERS = [random.Random(78).randrange(R) for _ in range(11)]
GOLDEN = os.path.join(ROOT, "tests", "golden", "prove_without_interval.json")


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def tv(xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.int64, device="cuda")


def dev_scalars(vals):
    return torch.from_numpy(synth.scalars_from_ints(vals).view(np.int64)).cuda()


def build(engine, kind, values=GOOD, bounds=BOUNDS, comp=None):
    """mixed appends (a ladder range_check, scalar gadgets, a public input, batched gates), then the interval items"""
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
    comp.interval_gate_batch(w8, S(bounds[8][0][0]), S(bounds[8][0][1]), 8)
    first = comp.add_input_batch(dev_scalars(values[16]))
    comp.interval_gate_ragged_batch(tv(range(first, first + len(values[16]))), dev_scalars([b[0] for b in bounds[16]]),
                                    dev_scalars([b[1] for b in bounds[16]]), 16)
    for v, (lo, hi) in zip(values[62], bounds[62]):
        comp.interval_gate(comp.add_input(S(v)), S(lo), S(hi), 62)
    comp.sync()
    if kind == "no_spare_rows":
        x = comp.add_input(S(3))
        assert comp.circuit_size() <= SIZES[kind]
        while comp.circuit_size() < SIZES[kind]:
            comp.constrain_to_constant(x, S(3), None)
        comp.sync()
        assert comp.circuit_size() == SIZES[kind]
    assert 1 << (comp.circuit_size() - 1).bit_length() == SIZES[kind], comp.circuit_size()
    return comp


def moved(bits):
    """BOUNDS with one bound of an item of `bits` bits moved by one (GOOD still satisfies it)"""
    out = {b: list(v) for b, v in BOUNDS.items()}
    if bits == 8:
        out[8] = [(100, 301)] * 2  # (the batch's one pair: raised, 300 is a witness)
    elif bits == 16:
        out[16][0] = (1, 65535)
    else:
        out[62][0] = (5, 5 + 2**62 - 2)
    return out


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
def test_a_satisfied_circuit_verifies_and_a_moved_bound_is_rejected(world, blinding):
    kind, comp, ck, ok, vk, pre, pi, n = world
    proof = comp.prove(ck, b"plonk", pre, blinding=blinding)
    assert len(proof.to_bytes()) == 1040
    assert all_verifiers(proof, vk, pre, ok, pi, n) == {True}
    # the key of the same circuit built with one bound moved by one: the same witnesses satisfy it, its q_c column differs
    for bits in BOUNDS:
        other = build(comp.engine, kind, bounds=moved(bits))
        assert other.check() == -1 and other.circuit_size() == comp.circuit_size()
        pre_m = other.preprocessed_commitments(ck, n)
        other.close()
        assert pre_m["q_c"] != pre["q_c"] and pre_m["q_range"] == pre["q_range"]
        assert all_verifiers(proof, pg.VerifierKey(n, pre_m), pre_m, ok, pi, n) == {False}
    # another public input
    assert not proof.verify(vk, ok, {row: (v + 1) % R for row, v in pi.items()})


@pytest.mark.parametrize("blinding", [None, True])
@pytest.mark.parametrize("bits,side", [(8, "below"), (8, "above"), (16, "above"), (62, "below")])
def test_a_witness_outside_its_interval_is_rejected(engine, keys, world, blinding, bits, side):
    kind, _, ck, ok, vk, pre, pi, n = world
    values = {b: list(v) for b, v in GOOD.items()}
    lo, hi = BOUNDS[bits][-1]
    values[bits][-1] = (lo - 1) % R if side == "below" else (hi + 1) % R
    comp = build(engine, kind, values)
    assert comp.check() >= 3 and comp.copy_constraints_hold()
    assert comp.preprocessed_commitments(ck) == pre  # the same circuit: the verifier's key is the honest one
    proof = comp.prove(ck, b"plonk", pre, blinding=blinding)
    comp.close()
    assert all_verifiers(proof, vk, pre, ok, pi, n) == {False}


def circuit_without_interval_items(engine):
    """appends that existed before the gadget: a ladder range_check, a public input and range_gate items"""
    comp = pg.StandardComposer(engine, 1 << 10, 1 << 10)
    a = pg.AllocatedScalar.allocate(comp, S(100))
    comp.constrain_to_constant(pg.range_check(comp, S(3), S(200), a), S(1), None)
    comp.constrain_to_constant(comp.add_input(S(9)), S(20), S(11))
    first = comp.add_input_batch(dev_scalars([0, 255, 77]))
    comp.range_gate_batch(tv(range(first, first + 3)), 8)
    comp.range_gate(comp.add_input(S(2**62 - 1)), 62)
    comp.sync()
    return comp


@pytest.mark.parametrize("blinding", ["unblinded", "fixed_blinders"])
def test_a_circuit_without_interval_items_proves_to_the_recorded_bytes(engine, keys, blinding):
    """the golden file holds the two proofs as the commit before the gadget produced them (same circuit, key and blinders)"""
    ck, ok = keys
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["blinders"] == [hex(b) for b in BLINDERS] and golden["tau"] == hex(TAU)
    comp = circuit_without_interval_items(engine)
    pre = comp.preprocessed_commitments(ck)
    proof = comp.prove(ck, b"plonk", pre, blinding=None if blinding == "unblinded" else BLINDERS)
    assert proof.to_bytes().hex() == golden[blinding]
    n = 1 << (comp.circuit_size() - 1).bit_length()
    assert proof.verify(pg.VerifierKey(n, pre), ok, public_inputs(comp))
    comp.close()


def test_clear_witness_refreshes_in_place_and_the_proof_is_deterministic(engine, keys, world):
    kind, _, ck, ok, vk, pre, pi, n = world
    comp = build(engine, kind)
    rows = comp.circuit_size()
    comp.clear_witness()
    second = {8: [101, 299], 16: [0, R - 1 - 40000], 62: [5 + 2**62 - 1]}
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
    # a third set with a witness outside: still in place, and rejected
    comp.clear_witness()
    build(engine, kind, {**second, 62: [4]}, comp=comp)
    assert comp.refresh_stats() == (rows - 3, 0, True) and comp.check() >= 3
    assert all_verifiers(comp.prove(ck, b"plonk", pre), vk, pre, ok, pi, n) == {False}
    comp.close()
