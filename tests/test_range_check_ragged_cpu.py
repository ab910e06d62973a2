"""CPU: the range_check family with one (min, max) pair per item is declared by the header, exported by the built library
and bound by _lib.py with as many arguments as the header gives it (no compute: the GPU suite is
tests/test_gpu_range_check_ragged.py)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ("pg_range_check_ragged_plan", "pg_range_check_ragged_plan_async", "pg_range_check_ragged_batch",
          "pg_range_check_ragged_values_batch", "pg_composer_range_check_ragged_batch")


def declarations():
    """name -> parameter list of every function the header declares"""
    text = open(os.path.join(ROOT, "include", "plonk_gadgets_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(pg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}


def test_header_library_and_bindings_agree_on_the_family():
    from plonk_gadgets_amd import _lib
    decl = declarations()
    lib = _lib.load()
    for name in FAMILY:
        assert name in decl, f"{name} is not declared in include/plonk_gadgets_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES, f"{name} has no entry in _lib.SIGNATURES"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl[name]), (name, len(args), decl[name])
        assert getattr(lib, name).argtypes == args
        # scalars by value where the header says uint64_t, pointers everywhere else
        for ctype, param in zip(args, decl[name]):
            assert (ctype is C.c_uint64) == (param.startswith("uint64_t ") and "*" not in param), (name, param)
    # the siblings they mirror take the same arguments but for the second bound array
    for mine, sibling, extra in (("pg_range_check_ragged_plan", "pg_max_bound_ragged_plan", 0),
                                 ("pg_range_check_ragged_plan_async", "pg_max_bound_ragged_plan_async", 0),
                                 ("pg_range_check_ragged_batch", "pg_max_bound_ragged_batch", 1),
                                 ("pg_range_check_ragged_values_batch", "pg_max_bound_ragged_values_batch", 1),
                                 ("pg_composer_range_check_ragged_batch", "pg_composer_max_bound_ragged_batch", 1)):
        assert len(decl[mine]) == len(decl[sibling]) + extra, (mine, sibling)


def test_engine_and_composer_expose_the_python_forms():
    import plonk_gadgets_amd as pg
    for name in ("range_check_ragged_batch", "range_check_ragged_plan", "range_check_ragged_plan_async", "range_check_ragged_emit",
                 "range_check_ragged_values"):
        assert callable(getattr(pg.Engine, name)), name
    assert callable(pg.StandardComposer.range_check_ragged_batch)
