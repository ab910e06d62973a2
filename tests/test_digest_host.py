"""CPU: csrc/digest.hpp -- the 128-bit digest of the device arrays an append's rows depend on, which the preflight's kernels and the
composer share -- built by g++, once plainly optimised, once under ASan + UBSan, and run by tests/cpp/digest_host.cpp on fixed seeded
arrays of 1, 2, 63, 64, 65 and 1000 words: the digest is the same however the words are dealt to lanes and in whatever order they are
summed; it changes when one entry changes, two entries of an array change places, two arrays of a call change places, two items' bounds
change places or an entry moves between two arrays; the named salts differ pairwise.  And once with the header mutated -- the word's
position dropped from the formula -- to see that the distinctions notice and the partitions do not."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonk_gadgets_amd", "csrc")


def build_and_run(tmp_path, flags, include):
    exe = str(tmp_path / "digest_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", include, os.path.join(ROOT, "tests", "cpp", "digest_host.cpp"),
                                                                             "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitizers"])
def test_digest_properties(tmp_path, flags):
    p = build_and_run(tmp_path, flags, CSRC)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    # six sizes x (12 partitions + 4 distinctions, and 4 more from two words on) + 28 pairs of salts
    assert p.stdout.strip() == "ok %d" % (6 * 16 + 5 * 4 + 28), p.stdout


def test_the_build_lists_every_file_of_csrc():
    """digest.hpp joined csrc/ as a header of its own: a file there that the build's list misses is neither a reason to rebuild the
    library nor part of the hash of its sources"""
    from plonk_gadgets_amd import build
    assert sorted(os.listdir(CSRC)) == sorted(build.SOURCES + build.HEADERS)


def test_distinctions_notice_a_dropped_position(tmp_path):
    """the mutation: without the word's position in either mix, entries (and items' bounds) that change places digest alike -- the
    distinctions must fail, and nothing but them: the sums still do not depend on the lanes"""
    src = open(os.path.join(CSRC, "digest.hpp")).read()
    first, second = "digest_mix(at + salt)", " + at * 0xc4ceb9fe1a85ec53ull"
    assert src.count(first) == 1 and src.count(second) == 1
    mutant = tmp_path / "mutant"
    mutant.mkdir()
    (mutant / "digest.hpp").write_text(src.replace(first, "digest_mix(salt)").replace(second, ""))
    p = build_and_run(tmp_path, ["-O2"], str(mutant))
    assert p.returncode == 1, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l and not l.endswith("check(s) failed")]
    assert lines and all(l.startswith("distinction: ") and "exchanged" in l for l in lines), p.stdout
    print(p.stdout.splitlines()[-1])
