"""CPU: the wait-state audit of tests/test_carry_hazards.py over the kernels of csrc/g1_codec.hpp, by name: each of them is in
the disassembly, its carry chains read VCC (so the audit has something to look at), and no VALU in it reads an SGPR fewer than
two wait states after a VALU wrote it.  The file has no inline asm, so this holds as long as the compiler pads its own chains;
the test is what says so for this file if that ever changes."""
import os
import subprocess

import pytest

from test_carry_hazards import kernel_bodies, parse, valu_sgpr_effects, violations
from test_kernel_resources import LLVM, code_object

KERNELS = ("g1_decompress_kernel", "g1_check_kernel", "g1_compress_kernel")


def test_codec_kernels_pass_the_wait_state_audit(tmp_path):
    objdump = os.path.join(LLVM, "llvm-objdump")
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not found")
    asm = subprocess.run([objdump, "-d", code_object(tmp_path)], capture_output=True, text=True, check=True).stdout
    bodies = {name: body for name, body in kernel_bodies(asm) if any(k in name for k in KERNELS)}
    assert len(bodies) == len(KERNELS), sorted(bodies)
    for name, body in bodies.items():
        lines = body.split("\n")
        vcc_reads = 0
        for line in lines:
            p = parse(line)
            if p and p[0].startswith("v_") and "vcc_lo" in valu_sgpr_effects(*p)[1]:
                vcc_reads += 1
        assert vcc_reads > 50, (name, vcc_reads)
        bad = violations(lines)
        assert not bad, (name, len(bad), bad[:4])
