"""CPU: the two kernels of pg_plonk_sides (csrc/plonk_sides.hpp) are in the gfx950 code object of the built library, use no
scratch, and keep the registers and LDS DESIGN section 3.16 states (no GPU needed)."""
from test_kernel_resources import code_object_notes, kernels

# kernel -> (VGPRs at most, LDS bytes exactly).  The compiler reports 247 VGPRs and 18 944 B of LDS for plonk_sides_kernel: under 256
# registers, so two waves can share a SIMD, and 74 words x 64 lanes x 4 B of sponge memory, eight workgroups' worth in a CU's 160
# KiB.  plonk_sides_decode_kernel is g1_decode with the membership test, as g1_decompress_kernel is: 341 VGPRs (unified VGPR + AGPR
# count), above 256, so one wave per SIMD and the next step up is the file of 512; no LDS.
LIMITS = {
    "plonk_sides_kernel": (256, 74 * 64 * 4),
    "plonk_sides_decode_kernel": (512, 0),
}


def test_plonk_sides_kernels_fit_without_scratch(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    for sub, (vgpr, lds) in LIMITS.items():
        hits = {n: k for n, k in ks.items() if sub in n}
        assert len(hits) == 1, (sub, sorted(hits))
        for name, k in hits.items():
            assert k["scratch"] == 0, (name, k)
            assert k["vgpr"] <= vgpr, (name, k)
            assert k["lds"] == lds, (name, k)
