"""A test-only TRAPDOOR verifier of plonk_gadgets_amd's proofs, in Python integers over tests/g1_model.py.

It knows the development SRS's secret tau, so each KZG pairing check e(W, [tau - x]_2) = e(F, [1]_2) becomes the G1 identity
(tau - x) W = F.  That is what a pairing verifier concludes too, so a proof it accepts is one a production verifier (out of scope
here) would accept, and it rejects what one would reject, as long as the prover does not know tau.

verify() recomputes the challenges with the same transcript, PI(xi) from the dense public-input vector by Lagrange
evaluation, t(xi) from the identity N(xi) = t(xi) Z_H(xi), builds [r] from the preprocessed commitments and [t] from
t_1 .. t_4, and checks the two openings (at xi with v, at xi omega with v')."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_model as G  # noqa: E402

from plonk_gadgets_amd.transcript import Transcript  # noqa: E402

R = G.R_FR
K = (1, 7, 13, 17)
ROOT_OF_UNITY = 0x16A2A19EDFE81F20D09B681922C813B4B63683508C2280B93829971F439F0D2B
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_4", "q_arith", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add")
SIGMAS = ("left_sigma", "right_sigma", "out_sigma", "fourth_sigma")
COMMITMENTS = ("a_comm", "b_comm", "c_comm", "d_comm", "z_comm", "t_1_comm", "t_2_comm", "t_3_comm", "t_4_comm", "w_z_comm",
               "w_zw_comm")
EVALUATIONS = ("a_eval", "b_eval", "c_eval", "d_eval", "a_next_eval", "b_next_eval", "d_next_eval", "q_arith_eval", "q_c_eval",
               "q_l_eval", "q_r_eval", "left_sigma_eval", "right_sigma_eval", "out_sigma_eval", "lin_poly_eval", "perm_eval")


def pt(g1affine):
    """a G1Affine -> g1_model's (x, y) or None"""
    return g1affine.to_ints()


def pi_at(pi: dict, xi: int, n: int, omega: int) -> int:
    """PI(xi) = sum_i pi_i L_i(xi), L_i(xi) = omega^i (xi^n - 1) / (n (xi - omega^i)); pi: row -> value (non-zero rows only)"""
    zh = (pow(xi, n, R) - 1) % R
    acc = 0
    for i, v in pi.items():
        wi = pow(omega, i, R)
        acc += v * wi * zh * pow(n * (xi - wi) % R, -1, R)
    return acc % R


def verify(proof, preprocessed: dict, pi: dict, n: int, tau: int, label=b"plonk") -> bool:
    """True iff both openings hold.  proof: plonk_gadgets_amd.Proof; preprocessed: name -> G1Affine (preprocessed_commitments);
    pi: row -> canonical public input (the verifier's own, rows of the padded circuit); n: the padded circuit size."""
    ev = {f: getattr(proof, f).to_int() for f in EVALUATIONS}
    cm = {f: getattr(proof, f) for f in COMMITMENTS}
    m = n.bit_length() - 1
    omega = pow(ROOT_OF_UNITY, 1 << (32 - m), R)
    # 1. the challenges
    tr = Transcript(label)
    tr.circuit_domain_sep(n)
    for name in SELECTORS + SIGMAS:
        tr.append_commitment(name.encode(), preprocessed[name])
    for lab, f in zip((b"w_l", b"w_r", b"w_o", b"w_4"), ("a_comm", "b_comm", "c_comm", "d_comm")):
        tr.append_commitment(lab, cm[f])
    beta = tr.challenge_int(b"beta")
    tr.append_scalar(b"beta", beta)
    gamma = tr.challenge_int(b"gamma")
    tr.append_commitment(b"z", cm["z_comm"])
    alpha = tr.challenge_int(b"alpha")
    for j in range(4):
        tr.append_commitment(b"t_%d" % (j + 1), cm["t_%d_comm" % (j + 1)])
    xi = tr.challenge_int(b"z")
    for f in EVALUATIONS:
        tr.append_scalar(f.encode(), ev[f])
    v = tr.challenge_int(b"aggregate_witness")
    tr.append_commitment(b"w_z", cm["w_z_comm"])
    v2 = tr.challenge_int(b"aggregate_witness")
    # 2.-3. PI(xi) and t(xi) from N(xi) = t(xi) Z_H(xi)
    if pow(xi, n, R) == 1:
        return False
    a, b, c, d = ev["a_eval"], ev["b_eval"], ev["c_eval"], ev["d_eval"]
    zw, qa = ev["perm_eval"], ev["q_arith_eval"]
    zh = (pow(xi, n, R) - 1) % R
    l1 = zh * pow(n * (xi - 1) % R, -1, R) % R
    p3 = (a + beta * ev["left_sigma_eval"] + gamma) * (b + beta * ev["right_sigma_eval"] + gamma) \
        * (c + beta * ev["out_sigma_eval"] + gamma) % R
    n_xi = (ev["lin_poly_eval"] + pi_at(pi, xi, n, omega) - alpha * p3 * (d + gamma) * zw - alpha * alpha * l1) % R
    t_eval = n_xi * pow(zh, -1, R) % R
    # 4. [r] from the preprocessed commitments and [z]; [t] from its parts
    zc = alpha
    for w, kj in zip((a, b, c, d), K):
        zc = zc * (w + beta * kj * xi + gamma) % R
    r_terms = [(qa * a * b, pt(preprocessed["q_m"])), (qa * a, pt(preprocessed["q_l"])), (qa * b, pt(preprocessed["q_r"])),
               (qa * c, pt(preprocessed["q_o"])), (qa * d, pt(preprocessed["q_4"])), (qa, pt(preprocessed["q_c"])),
               (zc + alpha * alpha * l1, pt(cm["z_comm"])), (-alpha * beta * zw * p3, pt(preprocessed["fourth_sigma"]))]
    xin = pow(xi, n, R)
    # 5. at xi: t, r, sigma_1..3, a, b, c, d, q_arith, q_c, q_l, q_r with v^0, v^1, ...
    terms = [(pow(xin, j, R), pt(cm["t_%d_comm" % (j + 1)])) for j in range(4)]
    terms += [(v * s % R, p) for s, p in r_terms]
    opened = [("left_sigma", "left_sigma_eval"), ("right_sigma", "right_sigma_eval"), ("out_sigma", "out_sigma_eval"),
              ("a_comm", "a_eval"), ("b_comm", "b_eval"), ("c_comm", "c_eval"), ("d_comm", "d_eval"), ("q_arith", "q_arith_eval"),
              ("q_c", "q_c_eval"), ("q_l", "q_l_eval"), ("q_r", "q_r_eval")]
    value = (t_eval + v * ev["lin_poly_eval"]) % R
    vi = v
    for name, f in opened:
        vi = vi * v % R
        terms.append((vi, pt(cm[name]) if name in cm else pt(preprocessed[name])))
        value = (value + vi * ev[f]) % R
    if not _opening_holds(terms, value, cm["w_z_comm"], xi, tau):
        return False
    # at xi omega: z, a, b, d with v'^0..3
    terms = [(1, pt(cm["z_comm"])), (v2, pt(cm["a_comm"])), (v2 * v2 % R, pt(cm["b_comm"])), (pow(v2, 3, R), pt(cm["d_comm"]))]
    value = (zw + v2 * ev["a_next_eval"] + v2 * v2 * ev["b_next_eval"] + pow(v2, 3, R) * ev["d_next_eval"]) % R
    return _opening_holds(terms, value, cm["w_zw_comm"], xi * omega % R, tau)


def _opening_holds(terms, value, witness, x, tau) -> bool:
    """(tau - x) [W] == sum_i c_i [P_i] - value G"""
    f = G.msm([c % R for c, _ in terms] + [(-value) % R], [p for _, p in terms] + [G.G])
    return G.mul((tau - x) % R, pt(witness)) == f
