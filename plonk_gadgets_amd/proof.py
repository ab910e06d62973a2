"""A PLONK proof of a StandardComposer's circuit: dusk-plonk 0.8's Prover::prove [DEP-RECALL] over the device rounds
(interpolation, the grand product, the quotient, evaluations, commitments and the openings of csrc/opening.hpp), with the
Fiat-Shamir transcript of transcript.py on the host.  DESIGN section 3.12.

Blinding is off by default, which keeps the proofs of earlier versions byte for byte: such a proof is sound
but NOT zero-knowledge.  prove(..., blinding=True) blinds the four wire polynomials and the grand product with 11 fresh scalars,
w_j + (b1 X + b0)(X^n - 1) and z + (b2 X^2 + b1 X + b0)(X^n - 1) (the PLONK paper's rounds 1 and 2; dusk-plonk 0.8 has none), so
that the commitments and evaluations a proof reveals are those of blinded polynomials; the quotient's parts are not blinded
separately (the paper's optional b10, b11 are left out).  The verifier does not change: a blinded proof is an ordinary proof.  The
arithmetic gate, the public inputs, the copy permutation and the three-wire range widget (range_gate, DESIGN section 3.19: its
term joins the quotient and r(X), no new evaluation or opening) are proven; circuits that use the logic or group-addition widgets
are refused (prover_polynomials)."""
from __future__ import annotations

import secrets
import time
from dataclasses import dataclass, fields

import torch

from .engine import DEFAULT_K, domain_generator
from .g1 import G1Affine, PolynomialDegreeTooLarge
from .scalar import BlsScalar
from .transcript import R, Transcript

COMMITMENTS = ("a_comm", "b_comm", "c_comm", "d_comm", "z_comm", "t_1_comm", "t_2_comm", "t_3_comm", "t_4_comm", "w_z_comm",
               "w_zw_comm")
EVALUATIONS = ("a_eval", "b_eval", "c_eval", "d_eval", "a_next_eval", "b_next_eval", "d_next_eval", "q_arith_eval", "q_c_eval",
               "q_l_eval", "q_r_eval", "left_sigma_eval", "right_sigma_eval", "out_sigma_eval", "lin_poly_eval", "perm_eval")
# r(X)'s columns, in the order of linearisation()
LINEARISATION_COLUMNS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "z", "fourth_sigma")


@dataclass
class Proof:
    """dusk-plonk 0.8's Proof: 11 commitments (G1Affine) and 16 evaluations (BlsScalar), serialised in that order as 11 x 48
    compressed bytes and 16 x 32 canonical little-endian bytes (1040 bytes)"""
    a_comm: G1Affine
    b_comm: G1Affine
    c_comm: G1Affine
    d_comm: G1Affine
    z_comm: G1Affine
    t_1_comm: G1Affine
    t_2_comm: G1Affine
    t_3_comm: G1Affine
    t_4_comm: G1Affine
    w_z_comm: G1Affine
    w_zw_comm: G1Affine
    a_eval: BlsScalar
    b_eval: BlsScalar
    c_eval: BlsScalar
    d_eval: BlsScalar
    a_next_eval: BlsScalar
    b_next_eval: BlsScalar
    d_next_eval: BlsScalar
    q_arith_eval: BlsScalar
    q_c_eval: BlsScalar
    q_l_eval: BlsScalar
    q_r_eval: BlsScalar
    left_sigma_eval: BlsScalar
    right_sigma_eval: BlsScalar
    out_sigma_eval: BlsScalar
    lin_poly_eval: BlsScalar
    perm_eval: BlsScalar

    SIZE = 11 * 48 + 16 * 32

    def to_bytes(self) -> bytes:
        out = b"".join(getattr(self, f).to_compressed() for f in COMMITMENTS)
        return out + b"".join(getattr(self, f).to_int().to_bytes(32, "little") for f in EVALUATIONS)

    @staticmethod
    def from_bytes(data: bytes) -> "Proof":
        """the inverse of to_bytes; ValueError on a wrong length, a bad point or a scalar not below r"""
        if len(data) != Proof.SIZE:
            raise ValueError(f"a proof is {Proof.SIZE} bytes, not {len(data)}")
        kw = {f: G1Affine.from_compressed(data[48 * i:48 * i + 48]) for i, f in enumerate(COMMITMENTS)}
        off = 48 * len(COMMITMENTS)
        for i, f in enumerate(EVALUATIONS):
            v = int.from_bytes(data[off + 32 * i:off + 32 * i + 32], "little")
            if v >= R:
                raise ValueError(f"{f} is not reduced below r")
            kw[f] = BlsScalar.from_int(v)
        return Proof(**kw)

    def verify(self, vk, ok, public_inputs=None, label=b"plonk") -> bool:
        """verifier.verify: True iff this proof verifies under the VerifierKey vk and the OpeningKey ok"""
        from .verifier import verify
        return verify(self, vk, ok, public_inputs, label)


assert [f.name for f in fields(Proof)] == list(COMMITMENTS + EVALUATIONS)


def linearisation(ev: dict, alpha: int, beta: int, gamma: int, xi: int, n: int, k=DEFAULT_K) -> list:
    """the coefficients rho_j (ints) of r(X) = sum_j rho_j s_j(X) over LINEARISATION_COLUMNS, from the evaluations `ev` (ints keyed
    as EVALUATIONS):
      r = q_arith(xi) (a b q_m + a q_l + b q_r + c q_o + d q_4 + q_c)
        + [alpha prod_j (w_j + beta k_j xi + gamma) + alpha^2 L1(xi)] z  -  alpha beta z(xi omega) P3 sigma_4,
    P3 = prod_{j < 3} (w_j + beta sigma_j(xi) + gamma), L1(xi) = (xi^n - 1) / (n (xi - 1))"""
    a, b, c, d = (ev[f] for f in ("a_eval", "b_eval", "c_eval", "d_eval"))
    qa = ev["q_arith_eval"]
    zh = (pow(xi, n, R) - 1) % R
    l1 = zh * pow(n * (xi - 1) % R, -1, R) % R
    p3 = 1
    for w, s in ((a, "left_sigma_eval"), (b, "right_sigma_eval"), (c, "out_sigma_eval")):
        p3 = p3 * (w + beta * ev[s] + gamma) % R
    num = alpha
    for w, kj in zip((a, b, c, d), k):
        num = num * (w + beta * kj * xi + gamma) % R
    rho = [qa * a * b, qa * a, qa * b, qa * c, qa * d, qa, num + alpha * alpha * l1, -alpha * beta * ev["perm_eval"] * p3]
    return [x % R for x in rho]


def range_rho(ev: dict, alpha: int) -> int:
    """rho_range, the coefficient of q_range(X) in r(X) for a circuit with range_gate items:
    alpha^3 delta(b - 4a) + alpha^4 delta(c - 4b) + alpha^5 delta(a_next - 4c), delta(f) = f (f - 1)(f - 2)(f - 3), from the
    evaluations a, b, c at xi and a at xi omega"""
    def delta(f):
        return f * (f - 1) * (f - 2) * (f - 3) % R
    a, b, c, an = (ev[f] for f in ("a_eval", "b_eval", "c_eval", "a_next_eval"))
    return (pow(alpha, 3, R) * delta(b - 4 * a) + pow(alpha, 4, R) * delta(c - 4 * b) + pow(alpha, 5, R) * delta(an - 4 * c)) % R


def _stacked(ts):
    """the equal-shape tensors as one int64[c, n, 4]: a view when they are consecutive in one buffer, else a copy"""
    n = ts[0].shape[0]
    if all(t.is_contiguous() for t in ts):
        v = ts[0].as_strided((len(ts), n, 4), (4 * n, 4, 1))
        if all(v[i].data_ptr() == t.data_ptr() for i, t in enumerate(ts)):
            return v
    return torch.stack(ts)


class _Phases:
    """wall-clock times of the prover's phases (the device synchronised at each mark) when a dict is given, else nothing"""

    def __init__(self, out, device):
        self.out, self.device = out, device
        if out is not None:
            torch.cuda.synchronize(device)
            self.t = time.perf_counter()

    def mark(self, name):
        if self.out is not None:
            torch.cuda.synchronize(self.device)
            t = time.perf_counter()
            self.out[name] = self.out.get(name, 0.0) + (t - self.t) * 1e3
            self.t = t


BLINDERS = 11  # a1 a0 b1 b0 c1 c0 d1 d0 z2 z1 z0
TAIL = 8       # zero rows behind every blinded column: the quotient's fourth part has n + 8 rows, and round 5 opens over n + 8


def _blinders(blinding):
    """prove's `blinding` -> None or 11 ints below r"""
    if blinding is None or blinding is False:
        return None
    if blinding is True:
        return [secrets.randbelow(R) for _ in range(BLINDERS)]
    b = [int(x) for x in blinding]
    if len(b) != BLINDERS:
        raise ValueError(f"blinding must be None, True or {BLINDERS} integers (a1 a0 b1 b0 c1 c0 d1 d0 z2 z1 z0), not {len(b)}")
    if any(not 0 <= x < R for x in b):
        raise ValueError("a blinder is not reduced below r")
    return b


def prove(composer, ck, label=b"plonk", preprocessed=None, timings: dict | None = None, blinding=None) -> Proof:
    """StandardComposer.prove: see there"""
    eng = composer.engine
    padded_n = composer._padded_n(None)
    m = padded_n.bit_length() - 1
    bl = _blinders(blinding)
    tail = 0 if bl is None else TAIL
    if bl is not None and padded_n < 8:
        raise ValueError(f"padded_n = {padded_n}: a blinded proof needs a circuit padded to at least 8 rows")
    if padded_n > ck.powers.shape[0]:
        raise PolynomialDegreeTooLarge(f"padded_n = {padded_n} > the key's {ck.powers.shape[0]} powers")
    if padded_n + tail > ck.powers.shape[0]:
        raise PolynomialDegreeTooLarge(f"a blinded proof needs padded_n + {TAIL} = {padded_n + TAIL} powers (the quotient's fourth "
                                       f"part has n + {TAIL} coefficients); the key has {ck.powers.shape[0]}")
    ph = _Phases(timings, eng.device)
    if preprocessed is None:
        preprocessed = composer.preprocessed_commitments(ck, padded_n)
        ph.mark("preprocess")
    tr = Transcript(label)
    tr.circuit_domain_sep(padded_n)
    for name in composer.SELECTORS + composer.SIGMAS:
        tr.append_commitment(name.encode(), preprocessed[name])
    S = BlsScalar.from_int

    # round 1: the wire polynomials
    wires = composer.wire_polynomials(padded_n, tail)
    if bl is not None:
        for j in range(4):
            eng.blind(wires[j], padded_n, bl[2 * j:2 * j + 2])
    ph.mark("round1_interpolate")
    w_comm = ck.commit(wires[:, :padded_n + 2] if tail else wires)
    del wires
    ph.mark("round1_msm")
    for lab, c in zip((b"w_l", b"w_r", b"w_o", b"w_4"), w_comm):
        tr.append_commitment(lab, c)
    beta = tr.challenge_int(b"beta")
    tr.append_scalar(b"beta", beta)
    gamma = tr.challenge_int(b"gamma")

    # round 2: the grand product (prover_polynomials also gives round 3's inputs)
    pp = composer.prover_polynomials(S(beta), S(gamma), padded_n, tail)
    if bl is not None:
        for j in range(4):
            eng.blind(pp["wires"][j], padded_n, bl[2 * j:2 * j + 2])
        eng.blind(pp["z"], padded_n, bl[8:11])
    ph.mark("round2_polynomials")
    z_comm = ck.commit(pp["z"][:padded_n + 3] if tail else pp["z"])
    ph.mark("round2_msm")
    tr.append_commitment(b"z", z_comm)
    alpha = tr.challenge_int(b"alpha")

    # round 3: the quotient
    if bl is None:
        t = eng.quotient(**pp, alpha=S(alpha), beta=S(beta), gamma=S(gamma))
        ph.mark("round3_quotient")
        t_comm = ck.commit(t)
    else:
        # t_1, t_2, t_3 of n rows and t_4 of n + 8, views of one int64[4n + 8, 4]
        tq = eng.quotient_blinded([pp["wires"][j, :padded_n + 2] for j in range(4)], pp["z"][:padded_n + 3], pp["sigmas"],
                                  pp["selectors"], pp["pi"], alpha=S(alpha), beta=S(beta), gamma=S(gamma), q_range=pp.get("q_range"))
        ph.mark("round3_quotient")
        t = [tq[j * padded_n:(j + 1) * padded_n] for j in range(3)] + [tq[3 * padded_n:]]
        t_comm = ck.commit(tq[:3 * padded_n].view(3, padded_n, 4)) + [ck.commit(t[3])]
    ph.mark("round3_msm")
    for i, c in enumerate(t_comm):
        tr.append_commitment(b"t_%d" % (i + 1), c)
    xi = tr.challenge_int(b"z")

    # round 4: evaluations at xi and xi omega, and r(xi)
    wires, z, sig, sel = pp["wires"], pp["z"], pp["sigmas"], pp["selectors"]
    xi_w = xi * domain_generator(m).to_int() % R
    names = eng.QUOTIENT_SELECTORS
    qe = dict(zip(names, (v.to_int() for v in eng.evaluate(_stacked([sel[s] for s in names]), xi))))
    we = [v.to_int() for v in eng.evaluate(wires, xi)]
    wn = [v.to_int() for v in eng.evaluate(wires, xi_w)]
    se = [v.to_int() for v in eng.evaluate(sig, xi)]
    z_xi = eng.evaluate(z, xi)[0].to_int()
    z_xiw = eng.evaluate(z, xi_w)[0].to_int()
    ev = {"a_eval": we[0], "b_eval": we[1], "c_eval": we[2], "d_eval": we[3], "a_next_eval": wn[0], "b_next_eval": wn[1],
          "d_next_eval": wn[3], "q_arith_eval": qe["q_arith"], "q_c_eval": qe["q_c"], "q_l_eval": qe["q_l"],
          "q_r_eval": qe["q_r"], "left_sigma_eval": se[0], "right_sigma_eval": se[1], "out_sigma_eval": se[2], "perm_eval": z_xiw}
    rho = linearisation(ev, alpha, beta, gamma, xi, padded_n)
    s_at_xi = [qe["q_m"], qe["q_l"], qe["q_r"], qe["q_o"], qe["q_4"], qe["q_c"], z_xi, se[3]]
    ev["lin_poly_eval"] = sum(r * s for r, s in zip(rho, s_at_xi)) % R
    q_range = pp.get("q_range")  # range_gate items: r(X) gains rho_range q_range(X)
    if q_range is not None:
        rho_range = range_rho(ev, alpha)
        ev["lin_poly_eval"] = (ev["lin_poly_eval"] + rho_range * eng.evaluate(q_range, xi)[0].to_int()) % R
    ph.mark("round4_evaluate")
    for f in EVALUATIONS:
        tr.append_scalar(f.encode(), ev[f])

    # round 5: the openings.  At xi: t (its parts weighted by xi^(jn)), r (folded into its columns' weights), sigma_1..3, a, b, c,
    # d, q_arith, q_c, q_l, q_r, with weights v^0, v^1, v^2, ...; a column that appears twice carries the sum of its weights.
    v = tr.challenge_int(b"aggregate_witness")
    cols, mu = {}, {}

    def put(key, tensor, weight):
        cols[key] = tensor
        mu[key] = (mu.get(key, 0) + weight) % R

    xin = pow(xi, padded_n, R)
    for j in range(4):
        put(("t", j), t[j], pow(xin, j, R))
    lin = dict(zip(LINEARISATION_COLUMNS, rho))
    for s in ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c"):
        put(s, sel[s], v * lin[s])
    put("z", z, v * lin["z"])
    put(("sigma", 3), sig[3], v * lin["fourth_sigma"])
    if q_range is not None:
        put("q_range", q_range, v * rho_range)
    opened = [sig[0], sig[1], sig[2], wires[0], wires[1], wires[2], wires[3], sel["q_arith"], sel["q_c"], sel["q_l"], sel["q_r"]]
    keys = [("sigma", 0), ("sigma", 1), ("sigma", 2), ("w", 0), ("w", 1), ("w", 2), ("w", 3), "q_arith", "q_c", "q_l", "q_r"]
    vi = v
    for key, tensor in zip(keys, opened):
        vi = vi * v % R
        put(key, tensor, vi)
    if bl is None:
        w_xi, _ = eng.open([cols[k_] for k_ in cols], [mu[k_] for k_ in cols], xi)
    else:
        # pg_poly_open wants one length for all its columns, and the witness is linear in them: the columns of n + 8 rows (t_4
        # and the tail-padded wires and z) open together, the columns of n rows together, and the two witnesses add up
        long_ = [k_ for k_ in cols if cols[k_].shape[0] == padded_n + TAIL]
        short = [k_ for k_ in cols if cols[k_].shape[0] == padded_n]
        assert len(long_) == 6 and len(long_) + len(short) == len(cols)
        w_xi, _ = eng.open([cols[k_] for k_ in long_], [mu[k_] for k_ in long_], xi)
        w_lo, _ = eng.open([cols[k_] for k_ in short], [mu[k_] for k_ in short], xi)
        w_xi[:padded_n] = eng.combine([w_xi[:padded_n], w_lo], [1, 1])
        del w_lo, tq
    del t, cols
    ph.mark("round5_open")
    w_z_comm = ck.commit(w_xi)
    del w_xi
    ph.mark("round5_msm")
    tr.append_commitment(b"w_z", w_z_comm)
    v2 = tr.challenge_int(b"aggregate_witness")
    w_xiw, _ = eng.open([z, wires[0], wires[1], wires[3]], [1, v2, v2 * v2 % R, pow(v2, 3, R)], xi_w)
    ph.mark("round5_open")
    w_zw_comm = ck.commit(w_xiw)
    ph.mark("round5_msm")
    tr.append_commitment(b"w_z_w", w_zw_comm)
    return Proof(*w_comm, z_comm, *t_comm, w_z_comm, w_zw_comm, *(S(ev[f]) for f in EVALUATIONS))
