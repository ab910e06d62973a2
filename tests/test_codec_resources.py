"""CPU: the kernels of csrc/g1_codec.hpp are in the built gfx950 code object, use no scratch memory and no LDS, and keep the
register counts DESIGN section 3.14 records (read off the code object the way tests/test_kernel_resources.py reads it; no GPU
needed).  The square root's window and the ladder's complete additions hold about 340 registers: above 256, so one wave per SIMD,
as for the MSM kernels; the encoder is small."""
from tests.test_kernel_resources import code_object_notes, kernels

# recorded from the build this was written against: decompress 343, check 346, compress 88, the first_bad initialiser 3.  The
# heavy kernels are past 256 either way (one wave per SIMD); 384 leaves the compiler some room and still catches a ladder or a
# square root that grew by a point's worth of registers.  128 (four waves per SIMD) for the encoder.
VGPR_BOUND = {"g1_decompress_kernel": 384, "g1_check_kernel": 384, "g1_compress_kernel": 128, "g1_first_bad_init_kernel": 16}


def test_codec_kernels_exist_and_do_not_spill(tmp_path, record_property):
    ks = kernels(code_object_notes(tmp_path))
    for name, bound in VGPR_BOUND.items():
        hits = {n: k for n, k in ks.items() if name in n}
        assert len(hits) == 1, f"{name}: {sorted(hits)}"
        for n, k in hits.items():
            record_property(name + "_vgpr", k["vgpr"])
            print(name, k)
            assert k["scratch"] == 0, (n, k)
            assert k["lds"] == 0, (n, k)
            assert k["vgpr"] <= bound, (n, k)
