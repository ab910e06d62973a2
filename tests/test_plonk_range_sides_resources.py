"""CPU: plonk_range_sides_kernel (csrc/plonk_sides.hpp, pg_plonk_range_sides) is in the gfx950 code object of the built library, uses
no scratch, and keeps the budget of plonk_sides_kernel that DESIGN sections 3.16 and 3.21 state (no GPU needed)."""
from test_kernel_resources import code_object_notes, kernels

# at most 256 VGPRs, so two waves can share a SIMD as for the 23-row kernel; the sponge memory and nothing else in LDS: 74 words x 64
# lanes x 4 B
VGPRS, LDS = 256, 74 * 64 * 4


def test_plonk_range_sides_kernel_fits_without_scratch(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    hits = {n: k for n, k in ks.items() if "plonk_range_sides_kernel" in n}
    assert len(hits) == 1, sorted(hits)
    for name, k in hits.items():
        print(name, k)
        assert k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= VGPRS, (name, k)
        assert k["lds"] == LDS == 18944, (name, k)
    # the decode kernel is shared with pg_plonk_sides: one kernel, the rows per proof its argument
    assert len([n for n in ks if "plonk_sides_decode_kernel" in n]) == 1
