"""GPU: the pairing verifier (plonk_gadgets_amd.verifier) end to end.

Every case tests/test_gpu_prove.py runs is run again THROUGH that module's own test functions, with its trapdoor verifier
wrapped: each call of plonk_verify_model.verify also runs pg.verify on the same proof, key, public inputs and label, and the two
verdicts must agree.  That covers every append kind, the reference's cases under keys of TRIM_LOG2 powers (accepted, and
rejected with the closing constant flipped), each tampering of test_tampered_proofs_are_rejected, the unsatisfied poly_gate
and the circuit padded to 2^20.  Then what a trapdoor cannot test: another tau's OpeningKey, keys rebuilt from bytes alone, a
commitment outside the subgroup, batches.  tau is used only through CommitKey.setup / OpeningKey.setup."""
import os
import sys

import pytest

import plonk_gadgets_amd as pg

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_prove as TP  # noqa: E402
import pairing_model as M  # noqa: E402
from test_g2_host import twist_point_outside_the_subgroup  # noqa: E402
from refcases import MAX_BOUND_CASES, MAYBE_EQUAL_CASES, RANGE_CHECK_CASES  # noqa: E402
from test_gpu_perm_product import KINDS, build  # noqa: E402

S = pg.BlsScalar.from_int
R = TP.R


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def big_key(engine):
    return pg.CommitKey.setup(engine, (1 << 20) - 1, S(TP.TAU))


@pytest.fixture(scope="module")
def opening_key(engine):
    ok = pg.OpeningKey.setup(engine, S(TP.TAU))
    yield ok
    ok.close()


@pytest.fixture
def compared(monkeypatch, opening_key):
    """wraps the trapdoor verifier test_gpu_prove calls: pg.verify must return what it returns; yields the list of verdicts"""
    model_verify = TP.V.verify
    seen = []

    def both(proof, preprocessed, pi, n, tau, label=b"plonk"):
        want = model_verify(proof, preprocessed, pi, n, tau, label)
        got = pg.verify(proof, pg.VerifierKey(n, preprocessed), opening_key, pi, label)
        assert got == want, (got, want)
        seen.append(want)
        return want
    monkeypatch.setattr(TP.V, "verify", both)
    yield seen
    assert seen, "the wrapped test verified nothing"


@pytest.mark.parametrize("kind", KINDS)
def test_every_append_kind(engine, big_key, compared, kind):
    TP.test_every_append_kind(engine, big_key, kind)


@pytest.mark.parametrize("max_range,witness,expected", MAX_BOUND_CASES)
def test_max_bound_cases(engine, compared, max_range, witness, expected):
    TP.test_max_bound_cases(engine, max_range, witness, expected)
    assert compared == [True, False]


@pytest.mark.parametrize("min_range,max_range,witness,expected", RANGE_CHECK_CASES)
def test_range_check_cases(engine, compared, min_range, max_range, witness, expected):
    TP.test_range_check_cases(engine, min_range, max_range, witness, expected)
    assert compared == [True, False]


@pytest.mark.parametrize("a,b,expected", MAYBE_EQUAL_CASES)
def test_maybe_equal_cases(engine, compared, a, b, expected):
    TP.test_maybe_equal_cases(engine, a, b, expected)


@pytest.mark.parametrize("sel", [0, 1])
def test_select_cases(engine, compared, sel):
    TP.test_select_zero_cases(engine, sel)
    TP.test_select_one_cases(engine, sel)


def test_is_non_zero_and_decomposition_cases(engine, compared):
    TP.test_is_non_zero_cases(engine)
    TP.test_scalar_decomposition_of_minus_100(engine)
    TP.test_the_verifier_side_circuit_has_the_same_preprocessed_commitments(engine)


def make_honest(engine, big_key, extra=9, more_gates=0):
    comp = build(engine, "allocated")
    for t in range(more_gates):  # (another circuit: other selectors, another verifier key)
        comp.constrain_to_constant(comp.add_input(S(t + 2)), S(t + 2), None)
    x = comp.add_input(S(extra))
    comp.constrain_to_constant(x, S(20), S(20 - extra))  # extra - 20 + PI = 0: one public input
    comp.sync()
    assert comp.check() == -1
    pre = comp.preprocessed_commitments(big_key)
    proof = comp.prove(big_key, b"plonk", pre)
    return comp, proof, pre


@pytest.fixture(scope="module")
def honest(engine, big_key):
    comp, proof, pre = make_honest(engine, big_key)
    yield comp, proof, pre
    comp.close()


def test_tampered_proofs_and_an_unsatisfied_gate(engine, big_key, compared, honest):
    TP.test_tampered_proofs_are_rejected(honest)
    assert compared.count(True) == 0 and len(compared) == len(TP.V.EVALUATIONS) + 4 + 2
    TP.test_an_unsatisfied_poly_gate_is_rejected(engine, big_key)


def test_a_range_check_circuit_padded_to_2_20(engine, big_key, compared):
    TP.test_a_range_check_circuit_padded_to_2_20(engine, big_key)
    assert compared == [True]


# ---- what the trapdoor cannot test --------------------------------------------------------------------------------------------
def test_keys_wrong_tau_and_keys_from_bytes(engine, big_key, opening_key, honest):
    comp, proof, pre = honest
    pi = TP.public_inputs(comp)
    vk = comp.verifier_key(big_key)
    assert vk == pg.VerifierKey(TP.padded(comp), pre)
    assert proof.verify(vk, opening_key, pi)
    assert not proof.verify(vk, opening_key, pi, b"testing")
    other = dict(pi)
    row = next(iter(other))
    other[row] = (other[row] + 1) % R
    assert not proof.verify(vk, opening_key, other)
    assert not proof.verify(vk, opening_key, {})
    # another tau's opening key
    wrong = pg.OpeningKey.setup(engine, S(TP.TAU + 1))
    assert not proof.verify(vk, wrong, pi)
    wrong.close()
    # everything rebuilt from bytes: no tau in sight
    data = opening_key.to_bytes()
    assert len(data) == pg.OpeningKey.SIZE == 240
    ok2 = pg.OpeningKey.from_bytes(engine, data)
    assert ok2.to_bytes() == data and (ok2.g, ok2.h, ok2.tau_h) == (opening_key.g, opening_key.h, opening_key.tau_h)
    with pytest.raises(ValueError):
        pg.OpeningKey.from_bytes(engine, data[:-1])
    with pytest.raises(ValueError, match="subgroup"):  # g on the curve, outside G1
        pg.OpeningKey.from_bytes(engine, off_subgroup_point().to_compressed() + data[48:])
    x, y = twist_point_outside_the_subgroup()
    with pytest.raises(ValueError, match="subgroup"):  # h on the twist, outside G2: from bytes and built by hand
        pg.OpeningKey.from_bytes(engine, data[:48] + M.g2_compressed((x, y)) + data[144:])
    with pytest.raises(ValueError, match="subgroup"):
        pg.OpeningKey(engine, opening_key.g, pg.G2Affine.from_ints(x, y), opening_key.tau_h)
    vk2 = pg.VerifierKey.from_bytes(vk.to_bytes())
    assert pg.Proof.from_bytes(proof.to_bytes()).verify(vk2, ok2, pi)
    ok2.close()


def off_subgroup_point():
    """a point of y^2 = x^3 + 4 outside the order-r subgroup (the cofactor is ~2^126: almost every curve point is)"""
    from plonk_gadgets_amd.verifier import g1_in_subgroup
    x = 1
    while True:
        x += 1
        try:
            p = pg.G1Affine.from_compressed(bytes([0x80 | (x >> 376)]) + (x & ((1 << 376) - 1)).to_bytes(47, "big"))
        except ValueError:
            continue
        if not g1_in_subgroup(p):
            return p


def test_bad_points_are_rejected_without_raising(engine, big_key, opening_key, honest):
    comp, proof, pre = honest
    pi, vk = TP.public_inputs(comp), pg.VerifierKey(TP.padded(comp), pre)
    bad = pg.Proof.from_bytes(proof.to_bytes())
    bad.w_z_comm = off_subgroup_point()
    assert bad.verify(vk, opening_key, pi) is False
    bad = pg.Proof.from_bytes(proof.to_bytes())
    limbs = list(proof.a_comm.limbs)
    limbs[0] ^= 1
    bad.a_comm = pg.G1Affine(limbs)  # not on the curve
    assert bad.verify(vk, opening_key, pi) is False
    # limbs at or above p that are congruent to a valid point: pg_msm would refuse them, verify must say False
    P = pg.g1.P
    limbs = list(proof.b_comm.limbs)
    xm = sum(w << (64 * i) for i, w in enumerate(limbs[:6])) + P
    assert xm < 1 << 384
    bad = pg.Proof.from_bytes(proof.to_bytes())
    bad.b_comm = pg.G1Affine([(xm >> (64 * i)) & (2**64 - 1) for i in range(6)] + limbs[6:])
    assert bad.b_comm.to_ints() == proof.b_comm.to_ints()
    assert bad.verify(vk, opening_key, pi) is False
    badkey = dict(pre)
    badkey["q_m"] = off_subgroup_point()
    assert proof.verify(pg.VerifierKey(TP.padded(comp), badkey), opening_key, pi) is False


def test_batches(engine, big_key, opening_key):
    """64 proofs of 4 different circuits"""
    circuits = [make_honest(engine, big_key, extra=3 + j, more_gates=j) for j in range(4)]
    vks = [pg.VerifierKey(TP.padded(c), pre) for c, _, pre in circuits]
    assert len({vk.to_bytes() for vk in vks}) == 4
    pis = [TP.public_inputs(c) for c, _, _ in circuits]
    proofs, pvk, ppi = [], [], []
    for i in range(64):
        j = i % 4
        proofs.append(pg.Proof.from_bytes(circuits[j][1].to_bytes()))
        pvk.append(vks[j])
        ppi.append(pis[j])
    assert pg.verify_batch(proofs, pvk, opening_key, ppi)
    assert pg.verify_each(proofs, pvk, opening_key, ppi) == [True] * 64
    proofs[37].c_eval = proofs[37].c_eval + S(1)
    assert not pg.verify_batch(proofs, pvk, opening_key, ppi)
    assert pg.verify_each(proofs, pvk, opening_key, ppi) == [i != 37 for i in range(64)]
    for c, _, _ in circuits:
        c.close()
