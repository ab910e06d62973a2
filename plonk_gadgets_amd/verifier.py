"""The pairing-based verifier of proof.Proof: VerifierKey, verify, verify_batch, verify_each.  DESIGN section 3.13.

The algebra is dusk-plonk 0.8's Proof::verify [DEP-RECALL]: the transcript of prove() replayed, PI(xi) by Lagrange evaluation,
t(xi) from N(xi) = t(xi) Z_H(xi), [r] from the key's commitments with the proof's q_arith(xi), the two KZG openings (at xi and
xi omega) folded by the separation challenge u into ONE check
    e(W_xi + u W_xiw, [tau]_2) e(-(xi W_xi + u xi omega W_xiw + F - E g), [1]_2) = 1,   F = F_xi + u F_xiw,  E = E_xi + u E_xiw.
Both G1 arguments are linear combinations of the same ~22 points: one Engine.msm_segmented call (one segment, two scalar
columns) gives both, then one pg_pairing_check of two pairs.  Everything a proof can get wrong makes verify return False; it never raises for it.

Subgroup: G1Affine.from_compressed tests the curve equation only, so every commitment of a proof is tested here for r P = O,
by a Jacobian double-and-add over Python integers (about 4 ms per point, cached; the key's 15 commitments are tested once).
That is the simplest means this package has, not a fast one -- pg_msm sums, it cannot multiply eleven points by r separately
-- and about as costly as the MSM of a single verify; the first follow-up is the endomorphism test (Bowe, 2019: half the
doublings) or a batched r P through the device's G1 code.

verify_batch folds the proofs' two sides with 128-bit weights drawn from `secrets` AFTER the proofs are fixed: if some proof's
check e(A_i, [tau]_2) e(B_i, [1]_2) is not 1, the folded product is a non-zero polynomial of degree 1 in each weight over GT
(a group of prime order r), so it is 1 with probability at most 2^-128.  Weights from the OS rather than from a transcript over
all proofs: nothing then depends on every verifier hashing the same bytes in the same order, and a verifier has no reason to
be deterministic.  verify_each sums every proof's two sides in ONE pg_msm_segmented call (a segment per proof, DESIGN section
3.15) whose output goes straight into one pg_pairing_check of len(proofs) checks: the call that names the bad proof.

verify_encoded is verify_each for proofs given as bytes with the host out of the loop: pg_plonk_sides decodes
the commitments, replays the transcript from a per-key seed (VerifierKey.record) and writes every proof's fixed table of 23 rows on
the device, which the same segmented MSM and pairing check consume; `sides` above is the model it is tested against.  With
range_term=True it goes through pg_plonk_range_sides: a 24th row, rho_range [q_range], for proofs of circuits
with range_gate or interval_gate items."""
from __future__ import annotations

import ctypes as C
import functools
import secrets

import torch

from . import _lib
from .engine import DEFAULT_K, PgError, domain_generator
from .g1 import P, G1Affine, points_tensor
from .proof import COMMITMENTS, EVALUATIONS, Proof, range_rho
from .scalar import BlsScalar
from .transcript import R, Transcript

SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_4", "q_arith", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add")
SIGMAS = ("left_sigma", "right_sigma", "out_sigma", "fourth_sigma")
MAX_PAIRS = 8
# pg_plonk_sides: a proof's bytes, the rows of its table, the key commitments of rows 11..21 in their order
PROOF_BYTES = Proof.SIZE
SIDES_ROWS = 23
RANGE_SIDES_ROWS = 24  # pg_plonk_range_sides: row 23 is the key's q_range
SIDES_KEY_ROWS = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith", "left_sigma", "right_sigma", "out_sigma", "fourth_sigma")
SIDES_STATUS = ("PG_SIDES_OK", "PG_G1_BAD_ENCODING", "PG_G1_NOT_ON_CURVE", "PG_G1_NOT_IN_SUBGROUP", "PG_G1_NOT_REDUCED",
                "PG_SIDES_BAD_EVALUATION", "PG_SIDES_XI_IN_DOMAIN", "PG_SIDES_BAD_PUBLIC_INPUT", "PG_SIDES_BAD_KEY")


# ---- G1 membership ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1 << 16)
def _valid_limbs(limbs) -> bool:
    p = G1Affine(limbs).to_ints()
    if p is None:
        return True
    # Montgomery limbs at or above p stand for the same residue, but pg_msm refuses them: not a valid point here either
    if any(sum(w << (64 * i) for i, w in enumerate(limbs[6 * h:6 * h + 6])) >= P for h in (0, 1)):
        return False
    x, y = p
    if (y * y - x * x * x - 4) % P:
        return False
    # r P in Jacobian coordinates (dbl-2009-l, add-2007-bl with Z2 = 1)
    X, Y, Z = x, y, 1
    for bit in bin(R)[3:]:
        if Z:
            A, B = X * X % P, Y * Y % P
            Cq = B * B % P
            D = 2 * ((X + B) ** 2 - A - Cq) % P
            E = 3 * A % P
            X3 = (E * E - 2 * D) % P
            X, Y, Z = X3, (E * (D - X3) - 8 * Cq) % P, 2 * Y * Z % P
        if bit == "1":
            if not Z:
                X, Y, Z = x, y, 1
                continue
            ZZ = Z * Z % P
            U2, S2 = x * ZZ % P, y * Z * ZZ % P
            if U2 == X:
                if S2 != Y:
                    X, Y, Z = 1, 1, 0
                    continue
                return False  # (a doubling inside the ladder: only a point of tiny order gets here)
            H, r = (U2 - X) % P, (S2 - Y) % P
            HH = H * H % P
            HHH, V = H * HH % P, X * HH % P
            X3 = (r * r - HHH - 2 * V) % P
            X, Y, Z = X3, (r * (V - X3) - Y * HHH) % P, Z * H % P
    return Z == 0


def g1_in_subgroup(p: G1Affine) -> bool:
    """on y^2 = x^3 + 4 and of order dividing r (the identity included)"""
    return _valid_limbs(p.limbs)


# ---- the pairing check ------------------------------------------------------------------------------------------------------
def _prepared_array(prepared):
    arr = (C.c_void_p * len(prepared))(*[p._h for p in prepared])
    return arr


def pairing_check(engine, points: torch.Tensor, prepared) -> torch.Tensor:
    """pg_pairing_check: points int64[n_checks, n_pairs, 12] on the engine's device, prepared a list of n_pairs PreparedG2 ->
    uint8[n_checks], 1 where prod_j e(P_ij, Q_j) = 1"""
    if not (points.dim() == 3 and points.shape[2] == 12 and points.dtype == torch.int64 and points.device == engine.device
            and points.is_contiguous() and points.shape[1] == len(prepared)):
        raise ValueError("points must be a contiguous int64[n_checks, len(prepared), 12] tensor on the engine's device")
    out = torch.empty((points.shape[0],), dtype=torch.uint8, device=engine.device)
    st = engine._lib.pg_pairing_check(engine._h, points.data_ptr(), _prepared_array(prepared), points.shape[0], points.shape[1],
                                      out.data_ptr(), engine._stream())
    if st != 0:
        raise PgError(st, "pg_pairing_check")
    return out


def pairing_gt(engine, points: torch.Tensor, prepared) -> torch.Tensor:
    """pg_pairing_gt: the GT values (prod_j e(P_ij, Q_j))^3 as int64[n_checks, 72] (six Fq2 coefficients over w^k)"""
    if not (points.dim() == 3 and points.shape[2] == 12 and points.dtype == torch.int64 and points.device == engine.device
            and points.is_contiguous() and points.shape[1] == len(prepared)):
        raise ValueError("points must be a contiguous int64[n_checks, len(prepared), 12] tensor on the engine's device")
    out = torch.empty((points.shape[0], 72), dtype=torch.int64, device=engine.device)
    st = engine._lib.pg_pairing_gt(engine._h, points.data_ptr(), _prepared_array(prepared), points.shape[0], points.shape[1],
                                   out.data_ptr(), engine._stream())
    if st != 0:
        raise PgError(st, "pg_pairing_gt")
    return out


# ---- the key ----------------------------------------------------------------------------------------------------------------
class VerifierKey:
    """the padded circuit size n and the 15 preprocessed commitments (SELECTORS then SIGMAS).  The transcript absorbs all 15;
    [r] uses q_m, q_l, q_r, q_o, q_4, q_c and fourth_sigma; the xi opening left / right / out_sigma, q_arith, q_c, q_l, q_r."""
    NAMES = SELECTORS + SIGMAS
    SIZE = 8 + 48 * len(NAMES)
    RECORD_SIZE = C.sizeof(_lib.PlonkKeyC)
    RANGE_RECORD_SIZE = C.sizeof(_lib.PlonkRangeKeyC)

    def __init__(self, n: int, commitments: dict):
        if n < 1 or n & (n - 1):
            raise ValueError("n must be a power of two")
        if set(commitments) != set(self.NAMES):
            raise ValueError("a verifier key holds exactly the 15 preprocessed commitments")
        self.n = int(n)
        self.commitments = {k: commitments[k] for k in self.NAMES}
        # tested once, here: verify() trusts its key
        self.valid = all(g1_in_subgroup(c) for c in self.commitments.values())
        self._seeds = {}

    def record(self, ok, label=b"plonk", range_term: bool = False) -> bytes:
        """the bytes of one pg_plonk_key for this key, the generator of the opening key `ok` and the transcript label: the
        STROBE state after the label, circuit_domain_sep(n) and the 15 commitments (computed once per label and kept), log2 n,
        omega, the 11 key points of the sides table, ok.g.  With range_term the 1488 bytes of a pg_plonk_range_key: the same
        record followed by the key's q_range commitment."""
        label = bytes(label)
        seed = self._seeds.get(label)
        if seed is None:
            tr = Transcript(label)
            tr.circuit_domain_sep(self.n)
            for name in self.NAMES:
                tr.append_commitment(name.encode(), self.commitments[name])
            st = tr.strobe
            seed = self._seeds[label] = (bytes(st.state), st.pos, st.pos_begin, st.cur_flags)
        rec = _lib.PlonkRangeKeyC() if range_term else _lib.PlonkKeyC()
        if range_term:
            rec.q_range = self.commitments["q_range"].c
        C.memmove(rec.state, seed[0], 200)
        rec.pos, rec.pos_begin, rec.cur_flags = seed[1:]
        rec.log2_n = self.n.bit_length() - 1
        rec.omega = domain_generator(rec.log2_n).c
        for k, name in enumerate(SIDES_KEY_ROWS):
            rec.points[k] = self.commitments[name].c
        rec.g = ok.g.c
        return bytes(rec)

    def to_bytes(self) -> bytes:
        return self.n.to_bytes(8, "little") + b"".join(self.commitments[k].to_compressed() for k in self.NAMES)

    @staticmethod
    def from_bytes(data: bytes) -> "VerifierKey":
        if len(data) != VerifierKey.SIZE:
            raise ValueError(f"a verifier key is {VerifierKey.SIZE} bytes, not {len(data)}")
        n = int.from_bytes(data[:8], "little")
        return VerifierKey(n, {k: G1Affine.from_compressed(data[8 + 48 * i:56 + 48 * i]) for i, k in enumerate(VerifierKey.NAMES)})

    def __eq__(self, other) -> bool:
        return isinstance(other, VerifierKey) and self.n == other.n and self.commitments == other.commitments


# ---- one proof's two sides ---------------------------------------------------------------------------------------------------
def _pi_at(pi: dict, xi: int, n: int, omega: int, zh: int) -> int:
    acc = 0
    for i, v in pi.items():
        wi = pow(omega, int(i), R)
        acc += int(v) * wi * zh * pow(n * (xi - wi) % R, -1, R)
    return acc % R


def _as_ints(public_inputs) -> dict:
    out = {}
    for i, v in (public_inputs or {}).items():
        out[int(i)] = v.to_int() if isinstance(v, BlsScalar) else int(v) % R
    return out


def sides(proof: Proof, vk: VerifierKey, ok, public_inputs, label=b"plonk", range_term: bool = False):
    """None when the proof is rejected before any pairing, else {point: [a, b]}: the check is
    e(sum a P, [tau]_2) e(sum b P, [1]_2) = 1.
    range_term: r(X)'s term of the range widget, rho_range [q_range] from the key -- what verify, verify_each
    and verify_batch ask for.  Without it (the default) the table is the one pg_plonk_sides builds, whose model this function is:
    23 rows, none for q_range."""
    if not vk.valid:
        return None
    cm = {f: getattr(proof, f) for f in COMMITMENTS}
    if not all(g1_in_subgroup(c) for c in cm.values()):
        return None
    ev = {f: getattr(proof, f).to_int() for f in EVALUATIONS}
    pre, n = vk.commitments, vk.n
    m = n.bit_length() - 1
    omega = domain_generator(m).to_int()
    tr = Transcript(label)
    tr.circuit_domain_sep(n)
    for name in SELECTORS + SIGMAS:
        tr.append_commitment(name.encode(), pre[name])
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
    tr.append_commitment(b"w_z_w", cm["w_zw_comm"])
    u = tr.challenge_int(b"seperation challenge")  # (dusk's spelling) [DEP-RECALL]

    xin = pow(xi, n, R)
    if xin == 1:
        return None
    a, b, c, d = ev["a_eval"], ev["b_eval"], ev["c_eval"], ev["d_eval"]
    zw, qa = ev["perm_eval"], ev["q_arith_eval"]
    zh = (xin - 1) % R
    l1 = zh * pow(n * (xi - 1) % R, -1, R) % R
    p3 = (a + beta * ev["left_sigma_eval"] + gamma) * (b + beta * ev["right_sigma_eval"] + gamma) \
        * (c + beta * ev["out_sigma_eval"] + gamma) % R
    n_xi = (ev["lin_poly_eval"] + _pi_at(_as_ints(public_inputs), xi, n, omega, zh) - alpha * p3 * (d + gamma) * zw
            - alpha * alpha * l1) % R
    t_eval = n_xi * pow(zh, -1, R) % R
    zc = alpha
    for w, kj in zip((a, b, c, d), (k.to_int() if isinstance(k, BlsScalar) else int(k) for k in DEFAULT_K)):
        zc = zc * (w + beta * kj * xi + gamma) % R

    out = {}

    def put(point, ca, cb):
        s = out.setdefault(point, [0, 0])
        s[0] = (s[0] + ca) % R
        s[1] = (s[1] + cb) % R

    # F_xi: t, v r, then sigma_1..3, a, b, c, d, q_arith, q_c, q_l, q_r with v^2 ..; the second side carries -F
    for j in range(4):
        put(cm["t_%d_comm" % (j + 1)], 0, -pow(xin, j, R))
    for coeff, point in ((qa * a * b, pre["q_m"]), (qa * a, pre["q_l"]), (qa * b, pre["q_r"]), (qa * c, pre["q_o"]), (qa * d, pre["q_4"]),
                         (qa, pre["q_c"]), (zc + alpha * alpha * l1, cm["z_comm"]), (-alpha * beta * zw * p3, pre["fourth_sigma"])):
        put(point, 0, -v * coeff)
    # a circuit with range_gate items: r gains rho_range [q_range].  A key whose q_range is the identity
    # gets no row for it: its table is what it was
    if range_term and not pre["q_range"].is_identity():
        put(pre["q_range"], 0, -v * range_rho(ev, alpha))
    value = (t_eval + v * ev["lin_poly_eval"]) % R
    vi = v
    for point, f in ((pre["left_sigma"], "left_sigma_eval"), (pre["right_sigma"], "right_sigma_eval"), (pre["out_sigma"], "out_sigma_eval"),
                     (cm["a_comm"], "a_eval"), (cm["b_comm"], "b_eval"), (cm["c_comm"], "c_eval"), (cm["d_comm"], "d_eval"),
                     (pre["q_arith"], "q_arith_eval"), (pre["q_c"], "q_c_eval"), (pre["q_l"], "q_l_eval"), (pre["q_r"], "q_r_eval")):
        vi = vi * v % R
        put(point, 0, -vi)
        value = (value + vi * ev[f]) % R
    # u F_xiw: z, a, b, d with v'^0..3
    vj = u
    for point, f in ((cm["z_comm"], "perm_eval"), (cm["a_comm"], "a_next_eval"), (cm["b_comm"], "b_next_eval"), (cm["d_comm"], "d_next_eval")):
        put(point, 0, -vj)
        value = (value + vj * ev[f]) % R
        vj = vj * v2 % R
    put(ok.g, 0, value)
    put(cm["w_z_comm"], 1, -xi)
    put(cm["w_zw_comm"], u, -u * xi * omega)
    return out


def _scalar_rows(values) -> list:
    rows = []
    for x in values:
        rows.append([w - (1 << 64) if w >> 63 else w for w in BlsScalar.from_int(x % R).limbs()])
    return rows


def _msm2(engine, table: dict) -> list:
    """the two sums of a {point: [a, b]} table: one pg_msm call with two scalar columns"""
    pts = list(table)
    cols = torch.tensor([_scalar_rows(table[p][0] for p in pts), _scalar_rows(table[p][1] for p in pts)], dtype=torch.int64,
                        device=engine.device).view(2, len(pts), 4)
    return engine.msm(points_tensor(pts, engine.device), cols)


def _msm2_segmented(engine, tables) -> torch.Tensor:
    """the two sums of every {point: [a, b]} table of `tables`: the points and both scalar columns of all of them in one upload,
    ONE pg_msm_segmented call with a segment per table -> int64[len(tables), 2, 12] on the device, as pairing_check takes it"""
    pts, ca, cb, offsets = [], [], [], [0]
    for table in tables:
        for p, (a, b) in table.items():
            pts.append(p)
            ca.append(a)
            cb.append(b)
        offsets.append(len(pts))
    n = len(pts)
    flat = [w - (1 << 64) if w >> 63 else w for p in pts for w in p.limbs]
    for rows in (_scalar_rows(ca), _scalar_rows(cb)):
        flat.extend(w for row in rows for w in row)
    buf = torch.tensor(flat, dtype=torch.int64).to(engine.device)
    return engine.msm_segmented(buf[:12 * n].view(n, 12), buf[12 * n:].view(2, n, 4), offsets)


def _check(engine, ok, pairs) -> list:
    """pairs: [(A, B)] -> [bool], one pg_pairing_check over all"""
    pts = points_tensor([p for ab in pairs for p in ab], engine.device).view(len(pairs), 2, 12)
    res = pairing_check(engine, pts, [ok.prepared_tau_h, ok.prepared_h])
    return [bool(x) for x in res.cpu().tolist()]


def verify(proof: Proof, vk: VerifierKey, ok, public_inputs=None, label=b"plonk") -> bool:
    """True iff the proof verifies under the verifier key vk and the OpeningKey ok, for the public inputs {row: value} (rows of
    the padded circuit; canonical integers or BlsScalars).  False -- never an exception -- for xi^n = 1, a commitment off the
    curve or outside the order-r subgroup, and any proof whose pairing check fails."""
    table = sides(proof, vk, ok, public_inputs, label, range_term=True)
    if table is None:
        return False
    # one segment of pg_msm_segmented, not pg_msm: 14.2 ms instead of 50.5 for these 22 points (DESIGN section 3.15,
    # profiles/r15_msm_segmented.json)
    res = pairing_check(ok.engine, _msm2_segmented(ok.engine, [table]), [ok.prepared_tau_h, ok.prepared_h])
    return bool(res.cpu().tolist()[0])


def _broadcast(x, n):
    return list(x) if isinstance(x, (list, tuple)) else [x] * n


def verify_each(proofs, vks, ok, public_inputs, label=b"plonk") -> list:
    """verify for every proof: one pg_msm_segmented call (a segment per proof, two columns) and one pg_pairing_check of
    len(proofs) checks on its output.  vks / public_inputs / label: one per proof, or one for all."""
    n = len(proofs)
    vks, pis, labels = _broadcast(vks, n), _broadcast(public_inputs, n), _broadcast(label, n)
    out, tables, where = [False] * n, [], []
    for i, proof in enumerate(proofs):
        table = sides(proof, vks[i], ok, pis[i], labels[i], range_term=True)
        if table is not None:
            tables.append(table)
            where.append(i)
    if tables:
        res = pairing_check(ok.engine, _msm2_segmented(ok.engine, tables), [ok.prepared_tau_h, ok.prepared_h])
        for i, good in zip(where, res.cpu().tolist()):
            out[i] = bool(good)
    return out


def _proof_bytes(proofs):
    """(n, a uint8 tensor of n x 1040 bytes -- on whatever device it was given -- or a bytes-like)"""
    if isinstance(proofs, torch.Tensor):
        if proofs.dtype != torch.uint8 or proofs.numel() % PROOF_BYTES:
            raise ValueError(f"a tensor of proofs is uint8[n, {PROOF_BYTES}]")
        return proofs.numel() // PROOF_BYTES, proofs.contiguous().view(-1)
    if isinstance(proofs, (bytes, bytearray, memoryview)):
        data = bytes(proofs)
    else:
        parts = []
        for p in proofs:
            try:
                parts.append(p.to_bytes())
            except (PgError, ValueError):  # limbs that have no encoding: all zeros decode to PG_G1_BAD_ENCODING
                parts.append(bytes(PROOF_BYTES))
        data = b"".join(parts)
    if len(data) % PROOF_BYTES:
        raise ValueError(f"{len(data)} bytes are not a whole number of {PROOF_BYTES}-byte proofs")
    return len(data) // PROOF_BYTES, data


def verify_encoded(proofs, vks, ok, public_inputs=None, label=b"plonk", return_status=False, range_term: bool = False):
    """verify_each for a batch given as BYTES, the sides built on the device (pg_plonk_sides).
    proofs: a bytes-like of n x 1040, a uint8[n, 1040] tensor on the host or the device, or a list of Proof (taken by their
    to_bytes).  vks / public_inputs / label: one per proof, or one for all.  One upload of the inputs (proofs, the records of
    the distinct (key, label) pairs, key indices and the public inputs as CSR arrays, in one buffer), one pg_plonk_sides, one
    pg_msm_segmented over the uniform offsets 23 i (which stages its n + 1 offsets itself: a second, small copy inside that
    call), one pg_pairing_check, (status == 0) & check on the device, one download -> [bool].  Never raises for a bad proof;
    ValueError only for a wrong total length.
    The answer is verify's, proof by proof, with one exception: a public-input row >= n.  sides / verify take omega^row for
    any row (row n is row 0 to them) and may accept; here such a proof is rejected with PG_SIDES_BAD_PUBLIC_INPUT.
    With return_status also the lists (status, where) of pg_plonk_sides (SIDES_STATUS names the values; a key that is not
    valid gives PG_SIDES_BAD_KEY).
    range_term: the whole batch goes through pg_plonk_range_sides: records of 1488 bytes, 24 rows a proof
    -- row 23 is rho_range [q_range], the range widget's term, what verify asks of `sides` -- and the offsets 24 i.  Keys with
    and without range_gate / interval_gate items can share such a call: an identity q_range gives an empty row.  Without it (the
    default) ValueError also for a key whose q_range commitment is not the identity: pg_plonk_key has 11 points and its table 23
    rows, none of them for that term."""
    engine = ok.engine
    n, data = _proof_bytes(proofs)
    if n == 0:
        return ([], [], []) if return_status else []
    vks, pis, labels = _broadcast(vks, n), _broadcast(public_inputs, n), _broadcast(label, n)
    if not range_term and any(not vk.commitments["q_range"].is_identity() for vk in vks):
        raise ValueError("a key with a live q_range (range_gate or interval_gate items): pg_plonk_sides builds no row for the range "
                         "term; pass range_term=True, or use verify_each")
    rows = RANGE_SIDES_ROWS if range_term else SIDES_ROWS
    table, records, key_index, bad_key = {}, [], [], []
    for i in range(n):
        k = (id(vks[i]), bytes(labels[i]))
        if k not in table:
            table[k] = len(records)
            records.append(vks[i].record(ok, k[1], range_term))
        key_index.append(table[k])
        if not vks[i].valid:
            bad_key.append(i)
    pi_off, pi_rows, pi_vals = [0], [], []
    for pi in pis:
        for row, val in _as_ints(pi).items():
            pi_rows.append(row)
            pi_vals.extend(BlsScalar.from_int(val % R).limbs())
        pi_off.append(len(pi_rows))

    # one host buffer, every section on a 16-byte boundary
    sections, size = [], 0

    def section(raw):
        nonlocal size
        raw = bytes(raw)
        sections.append((size, raw))
        size = (size + len(raw) + 15) // 16 * 16
        return sections[-1][0], len(raw)
    on_device = isinstance(data, torch.Tensor) and data.device == engine.device
    at = {}
    if not on_device:
        at["proofs"] = section(bytes(data.cpu().numpy()) if isinstance(data, torch.Tensor) else data)
    at["keys"] = section(b"".join(records))
    at["index"] = section((C.c_uint32 * n)(*key_index))
    if pi_rows:
        at["off"] = section((C.c_uint64 * (n + 1))(*pi_off))
        at["rows"] = section((C.c_uint64 * len(pi_rows))(*[r & ((1 << 64) - 1) for r in pi_rows]))
        at["vals"] = section((C.c_uint64 * len(pi_vals))(*pi_vals))
    host = bytearray(size)
    for off, raw in sections:
        host[off:off + len(raw)] = raw
    dev = torch.frombuffer(host, dtype=torch.uint8).to(engine.device)

    def view(name, dtype=torch.uint8):
        if name not in at:
            return None
        off, length = at[name]
        return dev[off:off + length].view(dtype)
    d_proofs = data if on_device else view("proofs")
    if d_proofs.data_ptr() % 16:
        d_proofs = d_proofs.clone()
    vals = view("vals", torch.int64)
    bases, scalars, status, where = engine.plonk_sides(d_proofs, view("keys"), view("index", torch.int32), view("off", torch.int64),
                                                       view("rows", torch.int64), vals.view(-1, 4) if vals is not None else None,
                                                       range_term=range_term)
    sums = engine.msm_segmented(bases, scalars, range(0, rows * n + 1, rows))
    good = pairing_check(engine, sums, [ok.prepared_tau_h, ok.prepared_h])
    verdict = ((status == 0) & (good != 0)).to(torch.uint8)
    verdict, status, where = torch.stack([verdict, status, where]).cpu().tolist()
    for i in bad_key:  # sides() trusts a key only if it is valid
        verdict[i], status[i], where[i] = 0, SIDES_STATUS.index("PG_SIDES_BAD_KEY"), 0
    out = [bool(x) for x in verdict]
    return (out, status, where) if return_status else out


def verify_batch(proofs, vks, ok, public_inputs, label=b"plonk") -> bool:
    """True iff every proof verifies (up to 2^-128): the proofs' sides folded with random 128-bit weights into one two-column MSM
    over all their points -- shared key commitments merged -- and ONE two-pair check.  An empty batch is True."""
    n = len(proofs)
    if n == 0:
        return True
    vks, pis, labels = _broadcast(vks, n), _broadcast(public_inputs, n), _broadcast(label, n)
    folded = {}
    for i, proof in enumerate(proofs):
        table = sides(proof, vks[i], ok, pis[i], labels[i], range_term=True)
        if table is None:
            return False
        rho = 1 if i == 0 else secrets.randbits(128) | 1
        for point, (ca, cb) in table.items():
            s = folded.setdefault(point, [0, 0])
            s[0] = (s[0] + rho * ca) % R
            s[1] = (s[1] + rho * cb) % R
    a, b = _msm2(ok.engine, folded)
    return _check(ok.engine, ok, [(a, b)])[0]
