"""CPU: the kernels the comparison gadget adds (csrc/compare_gate.hpp) are in the built gfx950 code object: exactly two
instantiations of the streaming emitter for CompareGateGD -- full emission and the values-only refresh; no structure-only form,
since every item creates Variables -- without scratch memory and within 128 VGPRs (four waves per SIMD, the condition RangeGateGD
and IntervalGateGD are held to).  DESIGN section 3.23 records the register counts."""
from tests.test_kernel_resources import code_object_notes, kernels


def test_compare_gate_kernels_exist_and_stay_within_their_resources(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    emit = {n: k for n, k in ks.items() if "emit_kernel" in n and "CompareGateGD" in n}
    for n, k in emit.items():
        print(n, k)
    assert len(emit) == 2, list(emit)
    for n, k in emit.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (n, k)
    # the sibling widgets' emitters are untouched: the new descriptor's name contains neither of theirs
    assert len([n for n in ks if "emit_kernel" in n and "RangeGateGD" in n]) == 3
    assert len([n for n in ks if "emit_kernel" in n and "IntervalGateGD" in n]) == 4
