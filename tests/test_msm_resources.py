"""CPU: the commitment kernels (csrc/msm.hpp) are in the gfx950 code object of the built library, use no scratch and no LDS,
and keep the register counts DESIGN section 3.11 states (no GPU needed)."""
from test_kernel_resources import code_object_notes, kernels

# kernel -> VGPRs at most (the unified VGPR + AGPR count of the code object's notes; 512 is the file of one wave)
LIMITS = {
    "msm_digits_kernel": 64,
    "msm_segsum_kernelILb1E": 384,
    "msm_segsum_kernelILb0E": 384,
    "msm_bucket_reduce_kernel": 384,
    "msm_window_kernel": 384,
    "msm_combine_kernel": 384,
    "g1_normalize_kernel": 256,
    "srs_table_kernel": 384,
    "srs_points_kernel": 320,
}


def test_commitment_kernels_fit_without_scratch(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    for sub, most in LIMITS.items():
        hits = {n: k for n, k in ks.items() if sub in n}
        assert hits, sub
        for name, k in hits.items():
            assert k["scratch"] == 0, (name, k)
            assert k["lds"] == 0, (name, k)
            assert k["vgpr"] <= most, (name, k)
