"""CPU: csrc/host_util.hpp's workspace layouts (pg::Carve) built by g++ -- once plainly optimised, once under ASan + UBSan --
and run by tests/cpp/carve_host.cpp: parts aligned, in order and apart, inside the measured total (the program writes every
byte of every part into a buffer of exactly that size), and the totals of pg_msm's and pg_poly_evaluate's workspaces equal to
the closed forms those calls allocated by before their layouts were written once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitizers"])
def test_carve_layouts(tmp_path, flags):
    exe = str(tmp_path / "carve_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "plonk_gadgets_amd", "csrc"),
                                                                             os.path.join(ROOT, "tests", "cpp", "carve_host.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.strip() == "ok 8", p.stdout
