"""CPU: the kernels of pg_msm_segmented (csrc/msm_small.hpp) are in the gfx950 code object of the built library, use no
scratch, and keep the registers and LDS DESIGN section 3.15 states (no GPU needed)."""
from test_kernel_resources import code_object_notes, kernels

# kernel -> (VGPRs at most, LDS bytes at most).  The compiler reports 355 VGPRs (unified VGPR + AGPR count) and 36 864 B of LDS for
# msm_seg_mul_kernel, 313 VGPRs and 12 288 B for msm_seg_sum_kernel.  Both are above 256 registers, the most that lets two waves share a
# SIMD's file of 512, so both run at one wave per SIMD and the next step up is the file itself: 512.  One wave per SIMD is four
# one-wave workgroups per CU, and LDS must not lower that: 160 KiB / 4 = 40 KiB per workgroup (the table is 3 slots x 192 B x 64
# lanes, the tree one point per lane).
LIMITS = {
    "msm_seg_mul_kernel": (512, 40 * 1024),
    "msm_seg_sum_kernel": (512, 40 * 1024),
}


def test_segmented_msm_kernels_fit_without_scratch(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    for sub, (vgpr, lds) in LIMITS.items():
        hits = {n: k for n, k in ks.items() if sub in n}
        assert hits, sub
        for name, k in hits.items():
            assert k["scratch"] == 0, (name, k)
            assert k["vgpr"] <= vgpr, (name, k)
            assert 0 < k["lds"] <= lds, (name, k)
