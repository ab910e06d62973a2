"""CPU: no parameter of the generated Rust declarations (bindings/rust/src/ffi.rs) is a Rust keyword -- a C parameter called
`where`, `in` or `type` would make the whole file a syntax error, and no Rust toolchain compiles it here -- and the generator
refuses to emit one."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_ffi as g  # noqa: E402


def test_no_parameter_is_a_rust_keyword():
    text = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    decls = re.findall(r"pub fn (pg_[a-z0-9_]+)\((.*?)\)(?: -> [^;]+)?;", text)
    assert len(decls) >= 150
    for name, args in decls:
        for arg in filter(None, (a.strip() for a in args.split(","))):
            ident = arg.split(":")[0].strip()
            assert re.fullmatch(r"[A-Za-z_][A-Za-z0-9_]*", ident) and ident not in g.RUST_KEYWORDS, (name, arg)
    assert "where_: *mut u8" in text  # pg_plonk_sides_host's last parameter


@pytest.mark.parametrize("word", ["where", "in", "type", "ref", "match", "self", "async", "try"])
def test_the_generator_escapes_keywords(word):
    assert word in g.RUST_KEYWORDS
    assert g.rust_arg("uint8_t *%s" % word) == "%s_: *mut u8" % word
    assert g.rust_arg("const pg_scalar *scalar") == "scalar: *const PgScalar"
