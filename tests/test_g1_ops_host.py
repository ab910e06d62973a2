"""CPU: the host forms of csrc/g1.hpp's group law (g1x_add, g1x_add_affine, g1x_dbl, g1x_dbl_affine, g1x_mul_small,
g1x_from_affine, g1a_neg) against tests/g1_model.py, over the corpus of tests/g1_ops_corpus.py -- the one that
tests/test_gpu_g1_device.py runs on the device.  tests/cpp/g1_host.cpp is built by g++, once plainly optimised and once under
ASan + UBSan, as a program of its own.  (Batch normalisation exists only as a kernel: it is left to the GPU test.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import g1_model as G  # noqa: E402
import g1_ops_corpus as K  # noqa: E402


def test_the_corpus_checks_what_it_says():
    """the yardstick itself: a lifted point is accepted under any z and refused beside another point, an unreduced limb or a
    ZZZ that does not belong to ZZ; the integer doubling gives 2P"""
    p, q = K.points()[0][3], K.points()[0][7]
    for z in (1, 2, K.P - 1, 0x1234567):
        raw = tuple(v * G.RQ % K.P for v in K.lift(p, z))
        assert K.xyzz_is(raw, p) and not K.xyzz_is(raw, q) and not K.xyzz_is(raw, None)
        assert not K.xyzz_is((raw[0] + K.P,) + raw[1:], p)
        assert not K.xyzz_is(raw[:3] + ((K.P - raw[3]) % K.P,), p)  # -ZZZ: ZZ^3 = ZZZ^2 still holds, y changes sign
        assert not K.xyzz_is(raw[:3] + ((raw[3] + 1) % K.P,), p)
        two = tuple(v * G.RQ % K.P for v in K.xyzz_dbl(K.lift(p, z)))
        assert K.xyzz_is(two, G.add(p, p)) and two[2] != G.RQ % K.P  # (2P, and not under ZZ = 1)
    assert K.xyzz_is((5, 6, 0, 7), None) and not K.xyzz_is((5, 6, 0, 7), p)


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]],
                ids=["plain", "sanitizers"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("g1_host") / "g1_host")
    subprocess.check_call(["g++", "-std=c++17"] + request.param + ["-I", os.path.join(ROOT, "plonk_gadgets_amd", "csrc"),
                                                                 os.path.join(ROOT, "tests", "cpp", "g1_host.cpp"), "-o", path])
    return path


@pytest.mark.parametrize("op", list(K.OPS), ids=K.NAMES)
def test_group_law_on_the_host(exe, tmp_path, op):
    a, b, k, want = K.corpus()[op]
    names = []
    for tag, arr in (("a", a), ("b", b), ("k", k)):
        if arr is None:
            names.append("-")
        else:
            names.append(str(tmp_path / tag))
            arr.tofile(names[-1])
    out = str(tmp_path / "out")
    p = subprocess.run([exe, str(op), str(len(want))] + names + [out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-2000:]
    got = np.fromfile(out, dtype=np.uint64).reshape(len(want), 12 if op == K.NEG_AFFINE else 24)
    bad = K.bad_rows(op, got, want)
    assert not bad, (K.NAMES[op], bad)
