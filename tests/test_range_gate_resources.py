"""CPU: the kernels the range widget adds (csrc/range_gate.hpp: range_patch_kernel, range_check_rows_kernel and the three
instantiations of the streaming emitter for RangeGateGD; csrc/quotient.hpp: quotient_range_kernel and
quotient_range_top_kernel) are in the built gfx950 code object; none uses scratch memory, and those that are not emitters use no
LDS either.  quotient_step_kernel keeps its six instantiations.  DESIGN section 3.19 records the register counts."""
from tests.test_kernel_resources import code_object_notes, kernels

PLAIN = ("range_patch_kernel", "range_check_rows_kernel", "quotient_range_kernel", "quotient_range_top_kernel")


def test_range_widget_kernels_exist_and_use_no_scratch_and_no_lds(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    for name in PLAIN:
        hits = {n: k for n, k in ks.items() if name in n}
        assert len(hits) == 1, (name, list(hits))
        for n, k in hits.items():
            print(n, k)
            assert k["scratch"] == 0, (n, k)
            assert k["lds"] == 0, (n, k)
            assert k["vgpr"] <= 256, (n, k)
    # the emitter: full emission, rows alone (items of two bits create no Variable) and values alone (a witness refresh)
    emit = {n: k for n, k in ks.items() if "emit_kernel" in n and "RangeGateGD" in n}
    assert len(emit) == 3, list(emit)
    for n, k in emit.items():
        print(n, k)
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (n, k)  # (the four waves per SIMD of the ladder emitters)
    assert len([n for n in ks if "quotient_step_kernel" in n]) == 6
