"""CPU: no VALU in the library's gfx950 code reads VCC or an SGPR fewer than two wait states after a VALU wrote it.

hipcc pads this hazard in the code it schedules (an `s_nop 1` in front of every `v_addc_co_u32` of a plain 128-bit add, on
gfx942 and gfx950), but it pads nothing inside an inline-asm string: csrc/fr.hpp's carry chains must carry their own wait
states.  A missing pad gives wrong carries on some waves of some launches, with no fault and no message, so the rule is
checked on the built code object rather than trusted to tests that feed values.

The scan is linear over each kernel's disassembly: one wait state per instruction, N + 1 for `s_nop N`.  Writes are the SGPR
results of VALU instructions (VOPC `_e32` to VCC, VOPC `_e64` and `v_readlane`/`v_readfirstlane` destinations, the carry-out
of `v_add_co`/`v_addc`/`v_sub*_co`/`v_mad_u64_u32`/`v_mad_i64_i32`/`v_div_scale`); reads are a VALU's SGPR operands, the
implicit VCC of `_e32` carry-in and `v_cndmask` forms included.  A scalar instruction that overwrites the SGPR in between
ends the hazard; so does the end of straight-line code (`s_branch`, `s_endpgm`)."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import LLVM, code_object

WAIT_STATES = 2
# VOP2/VOP3b forms whose second operand is an SGPR carry-out (or the sdst of v_div_scale)
CARRY_OUT = re.compile(r"^v_(add_co_u32|sub_co_u32|subrev_co_u32|addc_co_u32|subb_co_u32|subbrev_co_u32|mad_u64_u32|mad_i64_i32|"
                       r"div_scale_f32|div_scale_f64)(_e32|_e64)?$")
# _e32 forms that read VCC whether or not the disassembler prints it
IMPLICIT_VCC_READ = re.compile(r"^v_(addc_co_u32|subb_co_u32|subbrev_co_u32|cndmask_b32)_e32$")
SGPR_DEST = re.compile(r"^v_(cmp|cmpx)_\w+$|^v_readlane_b32$|^v_readfirstlane_b32$")
ENDS_FLOW = re.compile(r"^s_(branch|endpgm|setpc_b64|trap)$")
# SALU and scalar-memory forms whose first operand is a destination: a VALU read after them sees their value, not the VALU's
SALU_DEST = re.compile(r"^s_(mov|cmov|movk|cselect|and|or|xor|andn2|orn2|nand|nor|xnor|not|add|addc|sub|subb|addk|mulk|mul|lshl\w*|"
                       r"lshr|ashr|bfe|bfm|brev|bcnt0|bcnt1|ff0|ff1|flbit|sext|min|max|abs|absdiff|getpc|load|buffer_load|"
                       r"and_saveexec|or_saveexec|xor_saveexec)(_[a-z0-9]+)*$")


def sgprs(op):
    """the SGPR names an operand covers: s7 -> {s7}, s[4:5] -> {s4, s5}, vcc -> {vcc_lo, vcc_hi}; others -> {}"""
    op = op.strip()
    m = re.fullmatch(r"s(\d+)", op)
    if m:
        return {op}
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", op)
    if m:
        return {f"s{i}" for i in range(int(m.group(1)), int(m.group(2)) + 1)}
    if op == "vcc":
        return {"vcc_lo", "vcc_hi"}
    if op in ("vcc_lo", "vcc_hi"):
        return {op}
    return set()


def parse(line):
    """(mnemonic, [operands]) of a disassembly line, or None for a line that is no instruction"""
    text = line.split("//")[0].strip()
    if not text or text.endswith(":") or text.startswith("<"):
        return None
    parts = text.split(None, 1)
    ops = [o.strip() for o in re.split(r",(?![^\[]*\])", parts[1])] if len(parts) > 1 else []
    # drop modifiers (clamp, offset:..., neg(...)) that follow the operands
    ops = [o.split()[0] for o in ops if o]
    return parts[0], ops


def valu_sgpr_effects(mn, ops):
    """(SGPRs written, SGPRs read) by one VALU instruction"""
    writes, reads = set(), set()
    first_src = 1
    if CARRY_OUT.match(mn) and len(ops) >= 2 and sgprs(ops[1]):
        writes |= sgprs(ops[1])
        first_src = 2
    elif SGPR_DEST.match(mn) and ops and sgprs(ops[0]):
        writes |= sgprs(ops[0])
    for o in ops[first_src:]:
        reads |= sgprs(o)
    if IMPLICIT_VCC_READ.match(mn):
        reads |= {"vcc_lo", "vcc_hi"}
    return writes, reads


def violations(lines):
    """[(index, instruction text, register, wait states seen)], one per VALU that reads an SGPR too close to the VALU write of that SGPR"""
    out = []
    t = 0
    written = {}  # SGPR -> wait-state clock just after the VALU that wrote it
    for i, line in enumerate(lines):
        p = parse(line)
        if p is None:
            continue
        mn, ops = p
        if mn.startswith("v_"):
            writes, reads = valu_sgpr_effects(mn, ops)
            close = [(t - written[r], r) for r in sorted(reads) if r in written and t - written[r] < WAIT_STATES]
            if close:
                out.append((i, line.split("//")[0].strip(), close[0][1], close[0][0]))
            t += 1
            for w in writes:
                written[w] = t
            continue
        t += (int(ops[0], 0) + 1) if mn == "s_nop" and ops else 1
        if ENDS_FLOW.match(mn):
            written.clear()
        elif SALU_DEST.match(mn) and ops:
            for w in sgprs(ops[0]):
                written.pop(w, None)
    return out


def kernel_bodies(asm):
    bodies = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", asm)
    return list(zip(bodies[1::2], bodies[2::2]))


def test_audit_sees_an_unpadded_carry_and_accepts_a_padded_one():
    unpadded = """
        v_add_co_u32_e32 v0, vcc, v4, v0
        v_addc_co_u32_e32 v1, vcc, v5, v1, vcc
        v_cmp_ne_u32_e64 s[4:5], 0, v3
        v_cndmask_b32_e64 v2, 0, 1, s[4:5]
        v_mad_u64_u32 v[6:7], s[8:9], v2, v3, v[6:7]
        s_nop 0
        v_addc_co_u32_e64 v8, s[10:11], 0, v8, s[8:9]
        v_cmp_ne_u32_e32 vcc, 0, v9
        v_addc_co_u32_e32 v10, vcc, 0, v10
        v_cmp_ne_u32_e32 vcc, 0, v9
        s_and_b64 vcc_lo, s[4:5], s[0:1]
        v_cndmask_b32_e32 v39, v0, v42, vcc"""
    got = violations(unpadded.split("\n"))
    assert [(v[2], v[3]) for v in got] == [("vcc_hi", 0), ("s4", 0), ("s8", 1), ("vcc_hi", 0), ("vcc_hi", 1)], got
    padded = """
        v_add_co_u32_e32 v0, vcc, v4, v0
        s_nop 1
        v_addc_co_u32_e32 v1, vcc, v5, v1, vcc
        v_cmp_ne_u32_e64 s[4:5], 0, v3
        v_mov_b32_e32 v7, 0
        s_mov_b32 s6, 0
        v_cndmask_b32_e64 v2, 0, 1, s[4:5]
        v_mad_u64_u32 v[6:7], s[8:9], v2, v3, v[6:7]
        v_mad_u64_u32 v[6:7], s[12:13], v2, v3, v[6:7]
        v_mad_u64_u32 v[6:7], s[14:15], v2, v3, v[6:7]
        v_addc_co_u32_e64 v8, s[10:11], 0, v8, s[8:9]
        v_cmp_ne_u32_e32 vcc, 0, v9
        s_and_b64 vcc, s[4:5], s[0:1]
        v_cndmask_b32_e32 v39, v0, v42, vcc
        s_endpgm
        v_addc_co_u32_e32 v1, vcc, v5, v1, vcc"""
    assert violations(padded.split("\n")) == []


def test_no_valu_reads_an_sgpr_within_two_wait_states_of_its_valu_write(tmp_path):
    objdump = os.path.join(LLVM, "llvm-objdump")
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not found")
    asm = subprocess.run([objdump, "-d", code_object(tmp_path)], capture_output=True, text=True, check=True).stdout
    bodies = kernel_bodies(asm)
    assert len(bodies) > 100, len(bodies)
    vcc_reads, bad = 0, {}
    for name, body in bodies:
        lines = body.split("\n")
        for line in lines:
            p = parse(line)
            if p and p[0].startswith("v_") and "vcc_lo" in valu_sgpr_effects(*p)[1]:
                vcc_reads += 1
        v = violations(lines)
        if v:
            bad[name] = v
    # the audit has something to look at: the field arithmetic's carry chains read VCC on every product and sum
    assert vcc_reads > 10_000, vcc_reads
    summary = {n: (len(v), v[0][1]) for n, v in sorted(bad.items(), key=lambda kv: -len(kv[1]))[:8]}
    assert not bad, f"{sum(len(v) for v in bad.values())} reads in {len(bad)} kernels, e.g. {summary}"
