"""CPU: csrc/owners.hpp -- the owners of every device buffer, pinned buffer, stream and event of the host side -- built by g++
against the stand-in runtime of tests/cpp/stub, once plainly optimised, once under ASan + UBSan (LeakSanitizer with it), and run
by tests/cpp/owners_host.cpp: growth, refused growth, moves, and for the composer's column store every allocation and every copy
of a create and of each kind of grow failing in turn, after which the store is what it was and nothing is left alive.
And a search of csrc/: the runtime's allocate / free / create / destroy calls occur in owners.hpp alone."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonk_gadgets_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitizers"])
def test_owners(tmp_path, flags):
    exe = str(tmp_path / "owners_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags +
                          ["-I", os.path.join(ROOT, "tests", "cpp", "stub"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "owners_host.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert re.fullmatch(r"ok \d+", p.stdout.strip()), p.stdout


def test_only_the_owners_allocate_and_create():
    """the one search that shows the rule of DESIGN section 1: outside owners.hpp no line of csrc/ names one of these calls"""
    calls = re.compile(r"\bhip(Malloc|Free|HostMalloc|HostFree|EventCreate\w*|EventDestroy|StreamCreate\w*|StreamDestroy)\b")
    text = re.compile(r'"(\\.|[^"\\])*"|//.*')  # (error messages and comments may speak of them)
    found = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            hits = [f"{name}:{n}: {line.strip()}" for n, line in enumerate(f, 1) if calls.search(text.sub("", line))]
        if hits:
            found[name] = hits
    assert list(found) == ["owners.hpp"], "\n".join(h for name, hits in found.items() if name != "owners.hpp" for h in hits)
    assert len(found["owners.hpp"]) >= 8  # (the search finds what it looks for)
