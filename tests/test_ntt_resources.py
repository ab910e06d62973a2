"""CPU: the kernels of csrc/ntt.hpp are in the built gfx950 code object, use no scratch memory, and keep the registers and LDS
DESIGN section 3.9 claims (read off the code object the way tests/test_kernel_resources.py reads it; no GPU needed)."""
from tests.test_kernel_resources import code_object_notes, kernels

# LDS per workgroup: a pass holds a 1024-point tile and 512 roots (48 KiB, three workgroups per CU); the bit-reversal pass two
# 32 x 33-point tiles (66 KiB, two per CU)
LDS = {"ntt_pass_kernel": 48 * 1024, "ntt_reverse_kernel": 2 * 32 * 33 * 32}


def test_ntt_kernels_exist_and_do_not_spill(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    for name, lds in LDS.items():
        hits = {n: k for n, k in ks.items() if name in n}
        assert hits, f"{name} is not in the code object"
        for n, k in hits.items():
            assert k["scratch"] == 0, (n, k)
            assert k["vgpr"] <= 256, (n, k)
            assert k["lds"] <= lds, (n, k)
