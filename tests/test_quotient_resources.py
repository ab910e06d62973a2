"""CPU: the kernels of csrc/quotient.hpp are in the built gfx950 code object, use no scratch memory, at most 256 registers, and the
LDS DESIGN section 3.10 states (read off the code object the way tests/test_kernel_resources.py reads it; no GPU needed)."""
from tests.test_kernel_resources import code_object_notes, kernels

# LDS per workgroup: the pointwise steps and the combine none; the evaluation's two kernels one 256-entry reduction buffer (8 KiB)
LDS = {"quotient_step_kernel": 0, "quotient_combine_kernel": 0, "poly_eval_kernel": 256 * 32, "poly_eval_reduce_kernel": 256 * 32}


def test_quotient_kernels_exist_and_do_not_spill(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    steps = [n for n in ks if "quotient_step_kernel" in n]
    assert len(steps) == 6, steps  # one instantiation per pointwise step
    for name, lds in LDS.items():
        hits = {n: k for n, k in ks.items() if name in n}
        assert hits, f"{name} is not in the code object"
        for n, k in hits.items():
            assert k["scratch"] == 0, (n, k)
            assert k["vgpr"] <= 256, (n, k)
            assert k["lds"] <= lds, (n, k)
