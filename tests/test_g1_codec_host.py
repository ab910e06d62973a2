"""CPU: G1 ingestion on the host against tests/g1_codec_model.py, limb for limb and status for status.

Twice: through the C ABI's host-only entry points (pg_g1_from_compressed, pg_g1_check_host; pg_g1_to_compressed is their
inverse), and through a host build of csrc/g1_codec.hpp itself (tests/cpp/codec_host.cpp, g++ -- once plainly optimised, once
under ASan + UBSan), which also reaches the decode without the membership test, the encoder and the |u| P ladder.  The corpus
is g1_codec_model.corpus(): G and small multiples, the identity, both signs of y, x = p - 1 and x >= p, the compressed bit
clear, identity encodings with stray bits, x with no square root, the order-3 points (0, +-2), curve points from random x,
limbs at or above p -- and a few thousand random points of the subgroup."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import g1_codec_model as M  # noqa: E402
import g1_model as G  # noqa: E402

N_RANDOM = 3000


@pytest.fixture(scope="module")
def cases():
    """(encodings, [(point, status)] with and without the membership test, limb cases, their statuses, the random points)"""
    enc, limbs = M.corpus()
    walk = M.subgroup_walk(N_RANDOM, 0x51)
    want = [M.decode(e) for e in enc] + [(p, M.OK) for p in walk]
    want_nocheck = [M.decode(e, check_subgroup=False) for e in enc]
    enc = enc + [G.compressed(p) for p in walk]
    limbs = limbs + [G.point_limbs(p) for p in walk[:64]]
    return enc, want, want_nocheck, limbs, [M.check_limbs(l) for l in limbs], walk


def test_c_abi_host_entry_points_match_the_model(cases):
    from plonk_gadgets_amd import _lib
    lib = _lib.load()
    enc, want, _, limbs, want_status, walk = cases
    n = len(enc)
    data = (C.c_uint8 * (48 * n)).from_buffer_copy(b"".join(enc))
    out = (_lib.G1AffineC * n)()
    status = (C.c_uint8 * n)()
    assert lib.pg_g1_from_compressed(data, n, out, status) == 0
    for i, (pt, st) in enumerate(want):
        assert status[i] == st, (i, enc[i].hex(), M.STATUS_NAMES[status[i]], M.STATUS_NAMES[st])
        assert list(out[i].x) + list(out[i].y) == G.point_limbs(pt), (i, enc[i].hex())
    # what decoded encodes back to the same bytes (the existing host encoder)
    good = [i for i, (pt, st) in enumerate(want) if st == M.OK]
    back = (C.c_uint8 * 48)()
    for i in good[:200]:
        assert lib.pg_g1_to_compressed(C.byref(out[i]), 1, back) == 0 and bytes(back) == enc[i]
    # the check on limbs
    m = len(limbs)
    pts = (_lib.G1AffineC * m)()
    for i, l in enumerate(limbs):
        for j in range(6):
            pts[i].x[j], pts[i].y[j] = l[j], l[6 + j]
    st2 = (C.c_uint8 * m)()
    assert lib.pg_g1_check_host(pts, m, st2) == 0
    assert list(st2) == want_status, [(i, st2[i], w) for i, w in enumerate(want_status) if st2[i] != w]
    # NULL pointers with a count, and count = 0
    assert lib.pg_g1_from_compressed(None, 1, out, status) == 2 and lib.pg_g1_check_host(None, 1, st2) == 2
    assert lib.pg_g1_from_compressed(None, 0, None, None) == 0 and lib.pg_g1_check_host(None, 0, None) == 0


def hexes(limbs):
    return " ".join("%x" % w for w in limbs)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitizers"])
def test_host_build_matches_the_model(tmp_path, cases, flags):
    enc, want, want_nocheck, limbs, want_status, walk = cases
    lines, expect = [], []
    for e, (pt, st) in zip(enc, want):
        lines.append("dec 1 " + e.hex())
        expect.append("%x " % st + hexes(G.point_limbs(pt)))
    for e, (pt, st) in zip(enc, want_nocheck):
        lines.append("dec 0 " + e.hex())
        expect.append("%x " % st + hexes(G.point_limbs(pt)))
    for l, st in zip(limbs, want_status):
        lines.append("chk " + hexes(l))
        expect.append("%x" % st)
    for pt in [None, G.G, (0, 2)] + walk[:300]:
        lines.append("enc " + hexes(G.point_limbs(pt)))
        expect.append(G.compressed(pt).hex())
    for pt in [G.G, (0, 2), (0, M.P - 2)] + walk[:8] + [M.decode(enc[-N_RANDOM - 1], False)[0]]:  # (the last: a cofactor point)
        lines.append("mulu " + hexes(G.point_limbs(pt)))
        expect.append(hexes(G.point_limbs(G.mul(-M.U, pt))))
    path = tmp_path / "vectors.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "codec_host")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "plonk_gadgets_amd", "csrc"),
                                                           os.path.join(ROOT, "tests", "cpp", "codec_host.cpp"), "-o", exe])
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-2000:]
    rows = [r.strip() for r in p.stdout.strip().split("\n")]
    assert len(rows) == len(expect)
    bad = [(line[:60], row[:40], exp[:40]) for line, row, exp in zip(lines, rows, expect) if row != exp]
    assert not bad, (len(bad), bad[:6])
