"""CPU: the kernels of csrc/opening.hpp are in the built gfx950 code object, use no scratch memory, at most 256 registers, and
the LDS DESIGN section 3.12 states (read off the code object the way tests/test_kernel_resources.py reads it; no GPU needed)."""
from tests.test_kernel_resources import code_object_notes, kernels

# LDS per workgroup: the combine pass its 256-entry reduction buffer (8 KiB; the plain sum one entry), the carry scan the same,
# the quotient pass its tile of 2048 scalars padded by 16 bytes per run of 8 (68 KiB)
LDS = {"open_combine_kernel": 256 * 32, "open_carry_kernel": 256 * 32, "open_quotient_kernel": (2 * 2048 + 256) * 16}


def test_open_kernels_exist_and_do_not_spill(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    combine = [n for n in ks if "open_combine_kernel" in n]
    assert len(combine) == 2, combine  # with and without the tile totals
    for name, lds in LDS.items():
        hits = {n: k for n, k in ks.items() if name in n}
        assert hits, f"{name} is not in the code object"
        for n, k in hits.items():
            assert k["scratch"] == 0, (n, k)
            assert k["vgpr"] <= 256, (n, k)
            assert k["lds"] <= lds, (n, k)
