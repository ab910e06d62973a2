"""CPU: the two kernels pg_quotient_blinded adds (csrc/quotient.hpp: quotient_blind_kernel, the QS_BLIND step, and
quotient_top_kernel) are in the built gfx950 code object and use no scratch memory, no LDS and at most 256 registers; the steps of
pg_quotient keep theirs.  DESIGN section 3.17 records the counts."""
from tests.test_kernel_resources import code_object_notes, kernels

NEW = ("quotient_blind_kernel", "quotient_top_kernel")


def test_blinded_quotient_kernels_exist_and_use_no_scratch_and_no_lds(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    for name in NEW:
        hits = {n: k for n, k in ks.items() if name in n}
        assert len(hits) == 1, (name, list(hits))
        for n, k in hits.items():
            print(n, k)
            assert k["scratch"] == 0, (n, k)
            assert k["lds"] == 0, (n, k)
            assert k["vgpr"] <= 256, (n, k)
    # the longer QuotientChunk argument costs pg_quotient's steps nothing
    for n, k in ks.items():
        if "quotient_step_kernel" in n or "quotient_combine_kernel" in n:
            assert k["scratch"] == 0 and k["lds"] == 0 and k["vgpr"] <= 256, (n, k)
