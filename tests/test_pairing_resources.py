"""CPU: the pairing kernel's resources as DESIGN section 3.13 states them, read off the built code object: 385 registers
(AGPRs included), so a SIMD holds ONE wave and a CU one workgroup of 252 lanes = four waves, one per SIMD; 96 936 bytes of LDS
(42 checks x 4 Fq12 slots x 576 bytes, plus 42 flags); no scratch."""
from test_kernel_resources import code_object_notes, kernels


def test_pairing_check_kernel_resources(tmp_path):
    ks = {n: k for n, k in kernels(code_object_notes(tmp_path)).items() if "pairing_check_kernel" in n}
    assert len(ks) == 1, list(ks)
    k = next(iter(ks.values()))
    assert k["scratch"] == 0
    assert k["lds"] == 42 * 4 * 6 * 96 + 42 * 4 == 96936
    assert k["lds"] <= 160 * 1024  # one workgroup per CU is all the registers allow: LDS is not what limits residency
    # 385 as built (256 VGPRs + 129 AGPRs).  A compiler may move a few; at 256 or below a SIMD would hold two waves, and both the
    # residency DESIGN states and the workgroup shape chosen for it would have to be revisited
    assert 377 <= k["vgpr"] <= 392, k["vgpr"]
