"""CPU: what weighted_sum_ragged_batch adds to the library (csrc/weighted_sum.hpp): the header declares the call and its geometry
query and the built library exports both; the geometry is a power-of-two tile; and the kernels -- tile aggregates, the carry scan,
the writer in its two modes, and the validation pass -- are in the built gfx950 code object without scratch memory.  DESIGN section
3.22 records the register counts."""
import ctypes as C
import os
import re

from tests.test_kernel_resources import code_object_notes, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pg_composer_weighted_sum_ragged_batch", "pg_weighted_sum_geometry")


def test_header_declares_and_library_exports_the_call():
    from plonk_gadgets_amd import _lib
    header = open(os.path.join(ROOT, "include", "plonk_gadgets_hip.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"pg_status\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None


def test_geometry_is_a_power_of_two_tile():
    from plonk_gadgets_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    fn = lib.pg_weighted_sum_geometry
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    tile, per_pass = C.c_uint32(), C.c_uint32()
    assert fn(C.byref(tile), C.byref(per_pass)) == 0
    assert tile.value >= 2 and tile.value & (tile.value - 1) == 0, tile.value
    assert per_pass.value >= 1
    assert fn(None, C.byref(per_pass)) == 2 and fn(C.byref(tile), None) == 2


def test_weighted_sum_kernels_exist_without_scratch(tmp_path):
    ks = kernels(code_object_notes(tmp_path))
    for name, count in (("weighted_sum_tiles_kernel", 1), ("weighted_sum_carry_kernel", 1), ("weighted_sum_write_kernel", 2),
                        ("weighted_sum_check_kernel", 1)):
        hits = {n: k for n, k in ks.items() if name in n}
        assert len(hits) == count, (name, list(hits))
        for n, k in hits.items():
            print(n, k)
            assert k["scratch"] == 0, (n, k)
    # the writer in both modes: every column, and var_values alone (the template argument as the Itanium mangling spells it)
    writers = [n for n in ks if "weighted_sum_write_kernel" in n]
    assert len([n for n in writers if "Lb1E" in n]) == 1 and len([n for n in writers if "Lb0E" in n]) == 1, writers
