"""A second STROBE-128 / Merlin, written from the STROBE v1.0.2 specification (section 6: the duplex, beginOp, runF) and the semantics
of merlin's strobe.rs, in a different shape from plonk_gadgets_amd.transcript.Strobe128: the state is 25 integer lanes, an operation's
bytes are buffered and applied a block at a time, and the padding of a block (the byte pos_begin at `pos`, 0x04 after it, 0x80 at
byte 167) is one XOR of one integer.  It shares only keccak_f1600_lanes with the code under test, which hashlib pins.

The model is instrumented: every permutation is recorded with the byte that caused it (StrobeModel.events), and classes() names what
those bytes were.  The tests use that to assert that a family of transcripts really puts a block boundary on every kind of byte.

replay_sides() is verifier.sides' sequence of appends and challenges over a proof's 1040 bytes, for any transcript object (the
model's or plonk_gadgets_amd's); seed_sides() the part before it that VerifierKey.record keeps as a seed."""
from plonk_gadgets_amd.transcript import keccak_f1600_lanes

R_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
RATE = 166  # bytes of a block: 200 - 2 * 128 / 8 - 2
LANE = (1 << 64) - 1
FLAG_I, FLAG_A, FLAG_C, FLAG_T, FLAG_M, FLAG_K = 1, 2, 4, 8, 16, 32
ABSORB, OVERWRITE, SQUEEZE = 0, 1, 2


class StrobeModel:
    def __init__(self, protocol_label: bytes):
        self.lanes = [0] * 25
        self.pos = self.pos_begin = self.cur_flags = 0
        self.events = []  # ("block", op, kind, j, n) | ("forced", op, pos) | ("begin_at_zero", op)
        self.op = 0
        self._on_boundary = False  # the last byte applied ended a block, nothing since
        # F([1, R + 2, 1, 0, 1, 96] || "STROBEv1.0.2"), R + 2 = 168 the rate of the underlying sponge
        self._xor(0, bytes([1, RATE + 2, 1, 0, 1, 96]) + b"STROBEv1.0.2")
        self.lanes = keccak_f1600_lanes(self.lanes)
        self.meta_ad(protocol_label, False)

    def clone(self) -> "StrobeModel":
        c = StrobeModel.__new__(StrobeModel)
        c.__dict__.update(self.__dict__)
        c.lanes, c.events = list(self.lanes), list(self.events)
        return c

    # ---- the state as one 1600-bit integer ----------------------------------------------------------------------------------
    def _xor_int(self, v: int):
        for k in range(25):
            self.lanes[k] ^= (v >> (64 * k)) & LANE

    def _xor(self, at: int, data: bytes):
        self._xor_int(int.from_bytes(data, "little") << (8 * at))

    def _read(self, at: int, n: int) -> bytes:
        v = sum(lane << (64 * k) for k, lane in enumerate(self.lanes))
        return ((v >> (8 * at)) & ((1 << (8 * n)) - 1)).to_bytes(n, "little")

    def _clear(self, at: int, n: int):
        self._xor(at, self._read(at, n))

    def state_bytes(self) -> bytes:
        return self._read(0, 200)

    # ---- runF and the duplex ------------------------------------------------------------------------------------------------
    def _run_f(self):
        self._xor_int(self.pos_begin << (8 * self.pos) | 0x04 << (8 * (self.pos + 1)) | 0x80 << (8 * (RATE + 1)))
        self.lanes = keccak_f1600_lanes(self.lanes)
        self.pos = self.pos_begin = 0

    def _duplex(self, data: bytes, mode: int, kind: str, n=None) -> bytes:
        """`data` (zeros for a squeeze) in pieces that end where a block ends; `kind` and `n` only label the events"""
        out, i = bytearray(), 0
        n = len(data) if n is None else n
        while i < len(data):
            take = min(len(data) - i, RATE - self.pos)
            if mode != ABSORB:
                out += self._read(self.pos, take)
                self._clear(self.pos, take)
            if mode != SQUEEZE:
                self._xor(self.pos, data[i:i + take])
            self.pos += take
            i += take
            self._on_boundary = False
            if self.pos == RATE:
                self.events.append(("block", self.op, kind, i - 1, n))
                self._run_f()
                self._on_boundary = True
        return bytes(out)

    def _begin_op(self, flags: int, more: bool):
        if more:
            assert flags == self.cur_flags
            return
        assert not flags & FLAG_T
        self.op += 1
        if self._on_boundary and self.pos == 0 and self.pos_begin == 0:
            self.events.append(("begin_at_zero", self.op))
        frame = bytes([self.pos_begin, flags])
        self.pos_begin = self.pos + 1
        self.cur_flags = flags
        self._duplex(frame, ABSORB, "frame", flags)
        if flags & (FLAG_C | FLAG_K) and self.pos != 0:
            self.events.append(("forced", self.op, self.pos))
            self._run_f()

    def meta_ad(self, data: bytes, more: bool, kind="meta"):
        self._begin_op(FLAG_M | FLAG_A, more)
        self._duplex(data, ABSORB, kind)

    def ad(self, data: bytes, more: bool, kind="message"):
        self._begin_op(FLAG_A, more)
        self._duplex(data, ABSORB, kind)

    def prf(self, n: int, more: bool) -> bytes:
        self._begin_op(FLAG_I | FLAG_A | FLAG_C, more)
        return self._duplex(bytes(n), SQUEEZE, "squeeze")

    def key(self, data: bytes, more: bool):
        self._begin_op(FLAG_A | FLAG_C, more)
        self._duplex(data, OVERWRITE, "key")


class MerlinModel:
    """merlin::Transcript over StrobeModel, with the same methods as plonk_gadgets_amd.transcript.Transcript"""

    def __init__(self, label: bytes):
        self.strobe = StrobeModel(b"Merlin v1.0")
        self.append_message(b"dom-sep", label)

    def clone(self) -> "MerlinModel":
        t = MerlinModel.__new__(MerlinModel)
        t.strobe = self.strobe.clone()
        return t

    @property
    def events(self):
        return self.strobe.events

    def append_message(self, label: bytes, message: bytes):
        self.strobe.meta_ad(bytes(label), False, "label")
        self.strobe.meta_ad(len(message).to_bytes(4, "little"), True, "length")
        self.strobe.ad(bytes(message), False, "message")

    def append_u64(self, label: bytes, x: int):
        self.append_message(label, int(x).to_bytes(8, "little"))

    def append_scalar(self, label: bytes, s: int):
        self.append_message(label, (int(s) % R_FR).to_bytes(32, "little"))

    def append_commitment(self, label: bytes, point: bytes):
        self.append_message(label, point)

    def challenge_bytes(self, label: bytes, n: int) -> bytes:
        self.strobe.meta_ad(bytes(label), False, "label")
        self.strobe.meta_ad(n.to_bytes(4, "little"), True, "length")
        return self.strobe.prf(n, False)

    def challenge_int(self, label: bytes) -> int:
        return int.from_bytes(self.challenge_bytes(label, 64), "little") % R_FR

    def circuit_domain_sep(self, n: int):
        self.append_message(b"dom-sep", b"circuit_size")
        self.append_u64(b"n", n)


def classes(events) -> set:
    """the names of what the recorded permutations fell on:
    begin-first / flags / flags-C (the two framing bytes of beginOp; flags-C only when that operation ran exactly one permutation),
    label-first / -middle / -last, length-0 .. length-3, message-first / -middle / -last, squeeze, key (a one-byte label or message
    counts as its first and its last byte), begin-at-zero (an operation ended exactly on a block: the next beginOp starts at
    pos = 0 and absorbs old_begin = 0), forced-nonzero (the permutation the flag C forces at pos != 0)"""
    out = set()
    framing = {}
    for e in events:
        if e[0] != "begin_at_zero" and (e[0] == "forced" or e[2] == "frame"):
            framing[e[1]] = framing.get(e[1], 0) + 1
    for e in events:
        if e[0] == "begin_at_zero":
            out.add("begin-at-zero")
        elif e[0] == "forced":
            assert e[2] != 0
            out.add("forced-nonzero")
        else:
            _, op, kind, j, n = e
            if kind == "frame":
                if j == 0:
                    out.add("begin-first")
                elif n & FLAG_C:
                    if framing[op] == 1:
                        out.add("flags-C")
                else:
                    out.add("flags")
            elif kind == "length":
                out.add("length-%d" % j)
            elif kind in ("label", "message"):
                if j == 0:
                    out.add(kind + "-first")
                if j == n - 1:
                    out.add(kind + "-last")
                if 0 < j < n - 1:
                    out.add(kind + "-middle")
            else:
                out.add(kind)
    return out


# ---- verifier.sides' transcript ---------------------------------------------------------------------------------------------------
KEY_NAMES = (b"q_m", b"q_l", b"q_r", b"q_o", b"q_c", b"q_4", b"q_arith", b"q_range", b"q_logic", b"q_fixed_group_add",
             b"q_variable_group_add", b"left_sigma", b"right_sigma", b"out_sigma", b"fourth_sigma")
EVAL_NAMES = (b"a_eval", b"b_eval", b"c_eval", b"d_eval", b"a_next_eval", b"b_next_eval", b"d_next_eval", b"q_arith_eval", b"q_c_eval",
              b"q_l_eval", b"q_r_eval", b"left_sigma_eval", b"right_sigma_eval", b"out_sigma_eval", b"lin_poly_eval", b"perm_eval")
PROOF_BYTES, EVAL_AT = 1040, 528


def seed_sides(tr, n: int, key_commitments=None):
    """what comes before a key's seed: the circuit's domain separator and the key's 15 commitments (48 bytes each; only their
    length moves the block boundaries, so zeros stand in where none are given)"""
    tr.circuit_domain_sep(n)
    for k, name in enumerate(KEY_NAMES):
        tr.append_commitment(name, key_commitments[k] if key_commitments else bytes(48))
    return tr


def replay_sides(tr, data: bytes) -> list:
    """the seven challenges beta, gamma, alpha, xi, v, v', u of a proof's bytes, the transcript standing at the key's seed"""
    assert len(data) == PROOF_BYTES
    cm = [data[48 * j:48 * j + 48] for j in range(11)]
    out = []
    for j, lab in enumerate((b"w_l", b"w_r", b"w_o", b"w_4")):
        tr.append_message(lab, cm[j])
    out.append(tr.challenge_int(b"beta"))
    tr.append_message(b"beta", out[0].to_bytes(32, "little"))
    out.append(tr.challenge_int(b"gamma"))
    tr.append_message(b"z", cm[4])
    out.append(tr.challenge_int(b"alpha"))
    for j in range(4):
        tr.append_message(b"t_%d" % (j + 1), cm[5 + j])
    out.append(tr.challenge_int(b"z"))
    for k, name in enumerate(EVAL_NAMES):
        tr.append_message(name, data[EVAL_AT + 32 * k:EVAL_AT + 32 * k + 32])
    out.append(tr.challenge_int(b"aggregate_witness"))
    tr.append_message(b"w_z", cm[9])
    out.append(tr.challenge_int(b"aggregate_witness"))
    tr.append_message(b"w_z_w", cm[10])
    out.append(tr.challenge_int(b"seperation challenge"))
    return out


def sides_phase0_classes(label: bytes, n: int) -> set:
    """classes() of the permutations between a key's seed and the first challenge's forced permutation (the only part of the
    replay whose alignment depends on the label), with "commitment-first" / "commitment-last" for a proof commitment's bytes"""
    tr = seed_sides(MerlinModel(label), n)
    mark = len(tr.events)
    for lab in (b"w_l", b"w_r", b"w_o", b"w_4"):
        tr.append_message(lab, bytes(48))
    tr.challenge_bytes(b"beta", 64)
    ev = tr.events[mark:]
    cut = next(i for i, e in enumerate(ev) if e[0] == "forced" or (e[0] == "block" and e[2] == "frame" and e[3] == 1 and e[4] & FLAG_C))
    out = classes(ev[:cut + 1])
    return out | {c.replace("message", "commitment") for c in out if c.startswith("message")}
