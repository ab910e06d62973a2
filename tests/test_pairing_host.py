"""CPU: the tower, the prepared lines, the Miller loop and the final exponentiation of csrc/ in their HOST build
(tests/cpp/pairing_host.cpp, g++ -- once plainly optimised, once under ASan + UBSan) against tests/pairing_model.py, limb for
limb: every operation on an edge corpus (0, 1, u, p - 1 in each coefficient, elements of norm 1) and random elements, the
Frobenius maps against x -> x^p, the 68 line coefficients of prepared points, and the Miller and final values of several
(P, Q), two-pair products and identity points included.  The final value is the model's plain power cubed (HARD_C)."""
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import g1_model as G  # noqa: E402
import pairing_model as M  # noqa: E402

P, R = M.P, M.R


def hexes(limbs):
    return " ".join("%x" % w for w in limbs)


def f2_corpus(rng):
    edge = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1), (P - 1, P - 1), (1, 1), (P - 1, 1)]
    return edge + [(rng.randrange(P), rng.randrange(P)) for _ in range(24)]


def f12_corpus(rng):
    out = [list(M.F12_ZERO), list(M.F12_ONE)]
    for k in range(6):
        for c in ((1, 0), (0, 1), (P - 1, 0), (0, P - 1)):
            e = list(M.F12_ZERO)
            e[k] = c
            out.append(e)
    out.append([(P - 1, P - 1)] * 6)
    rnd = [[(rng.randrange(P), rng.randrange(P)) for _ in range(6)] for _ in range(6)]
    out += rnd
    # elements of norm 1 over Fq6: conj(f) / f
    out += [M.f12_mul(M.f12_conj(f), M.f12_inv(f)) for f in rnd[:3]]
    return out


def cases():
    """[(input line, expected limbs)]"""
    rng = random.Random(0x12)
    out = []
    c2 = f2_corpus(rng)
    ops2 = {"add": M.f2_add, "sub": M.f2_sub, "mul": M.f2_mul, "neg": lambda a, b: M.f2_neg(a), "sqr": lambda a, b: M.f2_sqr(a),
            "inv": lambda a, b: M.f2_inv(a), "conj": lambda a, b: M.f2_conj(a), "xi": lambda a, b: M.f2_mul_xi(a),
            "dbl": lambda a, b: M.f2_add(a, a)}
    for i, a in enumerate(c2):
        b = c2[(7 * i + 3) % len(c2)]
        for name, fn in ops2.items():
            out.append(("f2 %s %s %s" % (name, hexes(M.f2_limbs(a)), hexes(M.f2_limbs(b))), M.f2_limbs(fn(a, b))))
    c12 = f12_corpus(rng)
    ops12 = {"add": M.f12_add, "sub": M.f12_sub, "mul": M.f12_mul, "neg": lambda a, b: M.f12_neg(a), "sqr": lambda a, b: M.f12_sqr(a),
             "inv": lambda a, b: M.f12_inv(a), "conj": lambda a, b: M.f12_conj(a),
             "frob": lambda a, b: M.f12_pow(a, P), "frob2": lambda a, b: M.f12_frobenius(a, 2)}
    for i, a in enumerate(c12):
        b = c12[(5 * i + 2) % len(c12)]
        for name, fn in ops12.items():
            if name == "frob" and i % 4:
                fn = lambda a, b: M.f12_frobenius(a, 1)  # noqa: E731  (x -> x^p itself on every fourth element: it is slow)
            out.append(("f12 %s %s %s" % (name, hexes(M.f12_limbs(a)), hexes(M.f12_limbs(b))), M.f12_limbs(fn(a, b))))
        l0, l2, l3 = c2[i % len(c2)], c2[(i + 5) % len(c2)], rng.randrange(P) if i % 3 else (0, 1, P - 1)[i % 9 // 3]
        out.append(("sparse %s %s %s %s" % (hexes(M.f12_limbs(a)), hexes(M.f2_limbs(l0)), hexes(M.f2_limbs(l2)), hexes(G.fq_limbs(l3))),
                    M.f12_limbs(M.f12_mul_sparse(a, l0, l2, l3))))
    assert M.f12_frobenius(c12[-4], 2) == M.f12_pow(c12[-4], P * P)
    for k in (1, 2, R - 1, rng.randrange(R)):
        q = M.g2_mul(k, M.G2)
        out.append(("prep %s" % hexes(M.g2_limbs(q)), [w for c0, c2_ in M.g2_prepare(q) for w in M.f2_limbs(c0) + M.f2_limbs(c2_)]))
    pair_sets = [[(1, 1)], [(5, 7)], [(R - 1, 3)], [(2, 3), (R - 6, 1)], [(0, 4), (9, 2)], [(4, 5), (0, 1), (3, 11)]]
    for ps in pair_sets:
        pts = [(G.mul(a, G.G) if a else None, M.g2_mul(b, M.G2)) for a, b in ps]
        f = M.miller_loop([(p, M.g2_prepare(q)) for p, q in pts])
        final = M.f12_pow(M.final_exponentiation_plain(f), M.HARD_C)
        if ps == [(2, 3), (R - 6, 1)]:
            assert final == M.F12_ONE
        line = "pair %x " % len(ps) + " ".join(hexes(G.point_limbs(p)) + " " + hexes(M.g2_limbs(q)) for p, q in pts)
        out.append((line, M.f12_limbs(f) + M.f12_limbs(final)))
    return out


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    cs = cases()
    path = tmp_path_factory.mktemp("pairing_host") / "vectors.txt"
    path.write_text("\n".join(line for line, _ in cs) + "\n")
    return str(path), cs


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitizers"])
def test_host_build_matches_the_model(tmp_path, vectors, flags):
    path, cs = vectors
    exe = str(tmp_path / "pairing_host")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, "plonk_gadgets_amd", "csrc"),
                                                           os.path.join(ROOT, "tests", "cpp", "pairing_host.cpp"), "-o", exe])
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-2000:]
    rows = p.stdout.strip().split("\n")
    assert len(rows) == len(cs)
    bad = [line.split()[:2] for (line, want), row in zip(cs, rows) if [int(w, 16) for w in row.split()] != want]
    assert not bad, (len(bad), bad[:8])
