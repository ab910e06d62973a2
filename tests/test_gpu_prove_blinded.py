"""GPU: StandardComposer.prove(..., blinding=...) -- the wire polynomials and the grand product blinded -- under
the unchanged verifier.  Two circuits of a range check, scalar gadgets and a public input: one padded to 2^7 with spare rows, one
whose circuit_size() is exactly 2^6.  With blinding=True the proof verifies (Proof.verify, verify_batch, verify_encoded on its 1040
bytes) and a flipped byte in any commitment or evaluation is rejected; with fixed blinders two runs give the same bytes and blinders
of zero give the bytes of blinding=None; two sets of blinders give proofs whose 11 commitments and whose wire, z, linearisation and
quotient-dependent evaluations all differ while both verify, and whose selector and sigma evaluations are those of the public
polynomials at each proof's own xi; a_eval = a0(xi) + (b1 xi + b0)(xi^n - 1); and the errors."""
import os
import random
import sys

import numpy as np
import pytest

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth
from plonk_gadgets_amd.proof import COMMITMENTS, EVALUATIONS
from plonk_gadgets_amd.transcript import Transcript

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perm_product_model as PM  # noqa: E402

R = PM.Q
S = pg.BlsScalar.from_int
TAU = 0x5EED_7A1 ** 9 % R
SIZES = {"spare_rows": 1 << 7, "no_spare_rows": 1 << 6}
# the evaluations that depend on a blinded polynomial (through the wires, z, r or t) and those of public polynomials alone
BLINDED_EVALS = ("a_eval", "b_eval", "c_eval", "d_eval", "a_next_eval", "b_next_eval", "d_next_eval", "lin_poly_eval", "perm_eval")
PUBLIC_EVALS = {"q_arith_eval": ("selectors", "q_arith"), "q_c_eval": ("selectors", "q_c"), "q_l_eval": ("selectors", "q_l"),
                "q_r_eval": ("selectors", "q_r"), "left_sigma_eval": ("sigmas", 0), "right_sigma_eval": ("sigmas", 1),
                "out_sigma_eval": ("sigmas", 2)}
assert set(BLINDED_EVALS) | set(PUBLIC_EVALS) == set(EVALUATIONS)


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def blinders(seed):
    r = random.Random(seed)
    return [r.randrange(R) for _ in range(11)]


def build(engine, kind):
    comp = pg.StandardComposer(engine, 1 << 10, 1 << 10)
    a, b = pg.AllocatedScalar.allocate(comp, S(100)), pg.AllocatedScalar.allocate(comp, S(100))
    if kind == "spare_rows":
        res = pg.range_check(comp, S(50_000), S(250_000), pg.AllocatedScalar.allocate(comp, S(70_000)))
        comp.constrain_to_constant(res, S(1), None)
        comp.constrain_to_constant(pg.maybe_equal(comp, a, b), S(1), None)
        pg.is_non_zero(comp, a.var, S(100))
    else:
        res = pg.range_check(comp, S(3), S(200), a)
        comp.constrain_to_constant(res, S(1), None)
        comp.constrain_to_constant(pg.conditionally_select_zero(comp, b.var, comp.add_input(S(1))), S(100), None)
    comp.constrain_to_constant(comp.add_input(S(9)), S(20), S(11))  # 9 - 20 + PI(11) = 0: one public input
    comp.sync()
    if kind == "no_spare_rows":
        assert comp.circuit_size() <= SIZES[kind]
        x = comp.add_input(S(5))
        while comp.circuit_size() < SIZES[kind]:
            comp.constrain_to_constant(x, S(5), None)
            comp.sync()
        assert comp.circuit_size() == SIZES[kind]
    assert comp.check() == -1
    assert 1 << (comp.circuit_size() - 1).bit_length() == SIZES[kind], comp.circuit_size()
    return comp


@pytest.fixture(scope="module", params=list(SIZES))
def world(engine, request):
    """(composer, commit key of exactly padded_n + 8 powers, opening key, verifier key, preprocessed commitments, public inputs)"""
    comp = build(engine, request.param)
    n = SIZES[request.param]
    ck = pg.CommitKey.setup(engine, n + 7, S(TAU))  # max_degree n + 7: n + 8 powers
    assert ck.powers.shape[0] == n + 8
    ok = pg.OpeningKey.setup(engine, S(TAU))
    pre = comp.preprocessed_commitments(ck)
    dense = comp.construct_dense_pi_vec().cpu().numpy().view(np.uint64)
    pi = {i: synth.to_int(row) for i, row in enumerate(dense.tolist()) if any(row)}
    assert pi
    yield comp, ck, ok, pg.VerifierKey(n, pre), pre, pi, n
    ok.close()
    comp.close()


def xi_of(proof, pre, n, label=b"plonk"):
    """the evaluation challenge of the proof's own transcript"""
    tr = Transcript(label)
    tr.circuit_domain_sep(n)
    for name in pg.StandardComposer.SELECTORS + pg.StandardComposer.SIGMAS:
        tr.append_commitment(name.encode(), pre[name])
    for lab, f in zip((b"w_l", b"w_r", b"w_o", b"w_4"), COMMITMENTS[:4]):
        tr.append_commitment(lab, getattr(proof, f))
    beta = tr.challenge_int(b"beta")
    tr.append_scalar(b"beta", beta)
    tr.challenge_int(b"gamma")
    tr.append_commitment(b"z", proof.z_comm)
    tr.challenge_int(b"alpha")
    for j in range(4):
        tr.append_commitment(b"t_%d" % (j + 1), getattr(proof, "t_%d_comm" % (j + 1)))
    return tr.challenge_int(b"z")


def test_a_blinded_proof_verifies_and_a_flipped_byte_is_rejected(world):
    comp, ck, ok, vk, pre, pi, n = world
    timings = {}
    proof = comp.prove(ck, b"plonk", pre, timings, blinding=True)
    assert set(timings) >= {"round1_msm", "round3_quotient", "round5_open"}
    data = proof.to_bytes()
    assert len(data) == pg.Proof.SIZE == 1040 and pg.Proof.from_bytes(data) == proof
    assert proof.verify(vk, ok, pi)
    assert not proof.verify(vk, ok, {row: (v + 1) % R for row, v in pi.items()})
    assert pg.verify_batch([proof], vk, ok, pi)
    assert pg.verify_encoded(data, vk, ok, pi) == [True]
    # fresh randomness every time: another run differs in every commitment, and verifies too
    again = comp.prove(ck, b"plonk", pre, blinding=True)
    assert all(getattr(again, f) != getattr(proof, f) for f in COMMITMENTS)
    assert pg.verify_batch([proof, again], vk, ok, pi)
    # one byte flipped in each of the 11 commitments and 16 evaluations: all 27 rejected, the honest one among them accepted
    batch = [data]
    for i in range(len(COMMITMENTS)):
        bad = bytearray(data)
        bad[48 * i + 20] ^= 1
        batch.append(bytes(bad))
    for j in range(len(EVALUATIONS)):
        bad = bytearray(data)
        bad[48 * len(COMMITMENTS) + 32 * j + 3] ^= 1
        batch.append(bytes(bad))
    assert pg.verify_encoded(b"".join(batch), vk, ok, pi) == [True] + [False] * 27


def test_fixed_blinders_are_deterministic_and_zero_blinders_are_the_unblinded_proof(world):
    comp, ck, ok, vk, pre, pi, n = world
    b = blinders(1)
    first = comp.prove(ck, b"plonk", pre, blinding=b).to_bytes()
    assert comp.prove(ck, b"plonk", pre, blinding=tuple(b)).to_bytes() == first
    plain = comp.prove(ck, b"plonk", pre).to_bytes()
    assert comp.prove(ck, b"plonk", pre, blinding=None).to_bytes() == plain
    assert comp.prove(ck, b"plonk", pre, blinding=[0] * 11).to_bytes() == plain
    assert first != plain
    assert pg.verify_encoded(first + plain, vk, ok, pi) == [True, True]


def test_two_sets_of_blinders_differ_wherever_a_blinded_polynomial_shows(world):
    comp, ck, ok, vk, pre, pi, n = world
    eng = comp.engine
    sets = [blinders(2), blinders(3)]
    proofs = [comp.prove(ck, b"plonk", pre, blinding=b) for b in sets]
    assert pg.verify_each(proofs, vk, ok, pi) == [True, True]
    for f in COMMITMENTS + BLINDED_EVALS:
        assert getattr(proofs[0], f) != getattr(proofs[1], f), f
    # the selectors and sigmas are public: their evaluations are those of the unblinded polynomials at each proof's own xi (xi
    # itself depends on the blinded commitments, so the values differ between the proofs; nothing else about them does)
    pp = comp.prover_polynomials(S(1), S(2))
    a0 = comp.wire_polynomials()[0]
    for proof, b in zip(proofs, sets):
        xi = xi_of(proof, pre, n)
        for f, (key, j) in PUBLIC_EVALS.items():
            assert getattr(proof, f) == eng.evaluate(pp[key][j], xi)[0], f
        # a_eval = a0(xi) + (b1 xi + b0)(xi^n - 1)
        want = (eng.evaluate(a0, xi)[0].to_int() + (b[0] * xi + b[1]) * (pow(xi, n, R) - 1)) % R
        assert proof.a_eval.to_int() == want
        assert proof.a_eval != eng.evaluate(a0, xi)[0]
    # ... and the unblinded proof shows a0(xi) itself
    plain = comp.prove(ck, b"plonk", pre)
    assert plain.a_eval == eng.evaluate(a0, xi_of(plain, pre, n))[0]


def test_errors(engine, world):
    comp, ck, ok, vk, pre, pi, n = world
    # a key of exactly padded_n powers proves unblinded, and says what a blinded proof needs
    small = pg.CommitKey.setup(engine, n - 1, S(TAU))
    assert small.powers.shape[0] == n
    assert comp.prove(small, b"plonk", pre).verify(vk, ok, pi)
    with pytest.raises(pg.PolynomialDegreeTooLarge, match=r"padded_n \+ 8 = %d powers" % (n + 8)):
        comp.prove(small, b"plonk", pre, blinding=True)
    for bad in ([1] * 10, [1] * 12, [], [0] * 10 + [R], [-1] + [0] * 10):
        with pytest.raises(ValueError):
            comp.prove(ck, b"plonk", pre, blinding=bad)
    # a circuit padded to fewer than 8 rows
    tiny = pg.StandardComposer(engine, 1 << 8, 1 << 8)
    tiny.sync()
    assert tiny.circuit_size() <= 4
    with pytest.raises(ValueError, match="at least 8 rows"):
        tiny.prove(ck, blinding=True)
    tiny.close()
