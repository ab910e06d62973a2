"""CPU: the kernels the interval gadget adds (csrc/interval_gate.hpp) are in the built gfx950 code object: four instantiations of
the streaming emitter for IntervalGateGD -- full emission and the values-only refresh, with one pair of bounds for the call and
with a pair per item; no rows-only form, since every item creates Variables -- without scratch memory and within 128 VGPRs (four
waves per SIMD, as for RangeGateGD), and the one-lane-per-item validation of per-item bounds, which uses neither LDS nor scratch.
DESIGN section 3.20 records the register counts."""
from tests.test_kernel_resources import code_object_notes, kernels


def test_interval_gate_kernels_exist_and_stay_within_their_resources(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    emit = {n: k for n, k in ks.items() if "emit_kernel" in n and "IntervalGateGD" in n}
    for n, k in emit.items():
        print(n, k)
    assert len(emit) == 4, list(emit)
    for per_item in ("Lb0E", "Lb1E"):  # (the template argument as the Itanium mangling spells it)
        assert len([n for n in emit if per_item in n]) == 2, (per_item, list(emit))
    for n, k in emit.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (n, k)
    hits = {n: k for n, k in ks.items() if "interval_bounds_kernel" in n}
    assert len(hits) == 1, list(hits)
    for n, k in hits.items():
        print(n, k)
        assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= 128, (n, k)
    # the range widget's own emitters are untouched
    assert len([n for n in ks if "emit_kernel" in n and "RangeGateGD" in n]) == 3
