"""CPU: the kernels of csrc/permutation_product.hpp are in the built gfx950 code object and use no scratch memory (read off the
code object the way tests/test_kernel_resources.py reads it; no GPU needed)."""
from tests.test_kernel_resources import code_object_notes, kernels

NAMES = ("pp_tables_kernel", "pp_sigma_eval_kernel", "pp_ratio_kernel", "pp_carry_kernel", "pp_scan_kernel")


def test_permutation_product_kernels_exist_and_do_not_spill(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    for name in NAMES:
        hits = {n: k for n, k in ks.items() if name in n}
        assert hits, f"{name} is not in the code object"
        for n, k in hits.items():
            assert k["scratch"] == 0, (n, k)
            assert k["vgpr"] <= 256, (n, k)
    # the launch that carries the arithmetic: two workgroups of 256 lanes per CU by its registers, its LDS within a CU's share
    for n, k in ks.items():
        if "pp_ratio_kernel" in n:
            assert k["lds"] <= 64 * 1024, (n, k)
