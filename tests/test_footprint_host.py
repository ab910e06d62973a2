"""CPU: csrc/footprint.hpp -- which kernel pg_composer_permutation and pg_composer_materialize give a batched call's footprint, and
what an item of every kind weighs -- built by g++, once plainly optimised, once under ASan + UBSan, and run by
tests/cpp/footprint_host.cpp: a sweep over kind x uniform / ragged x tail x ladder length x shapes on every threshold against the
predicates those two calls spelled out before the header was written; the routes of the footprints real calls leave, written by
hand; the per-kind rows and Variables against the layout calls' closed forms.  And once with the header mutated -- `tail == 0`
dropped from the template route's condition -- to see that the sweep notices."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonk_gadgets_amd", "csrc")


def build_and_run(tmp_path, flags, include):
    exe = str(tmp_path / "footprint_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", include, os.path.join(ROOT, "tests", "cpp", "footprint_host.cpp"),
                                                                             "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitizers"])
def test_footprint_routes(tmp_path, flags):
    p = build_and_run(tmp_path, flags, CSRC)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    # 13 kinds x 2 x 3 tails x 5 ladder lengths x 33 shapes x 2 parities of the first row; 22 lines of the hand-written table
    assert p.stdout.strip() == "ok 25740 22", p.stdout


def test_sweep_notices_a_dropped_tail_condition(tmp_path):
    """the mutation: a template kind WITH a tail routed like one without must fail the sweep (and nothing but the sweep)"""
    src = open(os.path.join(CSRC, "footprint.hpp")).read()
    was = "if (is_template_kind(s.wire_kind) && s.tail == 0) return s.row_off ? PERM_TEMPLATE_RAGGED : PERM_TEMPLATE;"
    assert src.count(was) == 1
    mutant = tmp_path / "mutant"
    mutant.mkdir()
    (mutant / "footprint.hpp").write_text(src.replace(was, was.replace(" && s.tail == 0", "")))
    p = build_and_run(tmp_path, ["-O2"], str(mutant))
    assert p.returncode == 1, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l and not l.endswith("check(s) failed")]
    assert lines and all(l.startswith("sweep: ") and " tail 0 " not in l for l in lines), p.stdout
    print(p.stdout.splitlines()[-1])
