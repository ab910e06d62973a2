"""The group-law corpus of csrc/g1.hpp, shared by tests/test_gpu_g1_device.py (the device forms) and tests/test_g1_ops_host.py
(the host forms): operands as raw Montgomery limbs, and what tests/g1_model.py says each result is.

Points are k G for k in {1, 2, 3, r - 1, r - 2} and 60 random k; an affine (x, y) is lifted to XYZZ as (x z^2, y z^3, z^2, z^3)
for z in {1, 2, p - 1} and random z.  The identity appears as all zeros and as ZZ = 0 beside non-zero X, Y and ZZZ.  A result
(X, Y, ZZ, ZZZ) is right when its limbs are reduced and, out of Montgomery form, either ZZ = 0 and the model says identity, or
ZZ^3 = ZZZ^2 and (X / ZZ, Y / ZZZ) is the model's affine point."""
import functools
import random

import numpy as np

import g1_codec_model as CM
import g1_model as G

P, R = G.P, G.R_FR
RINV = pow(G.RQ, -1, P)
ADD, ADD_AFFINE, DBL, DBL_AFFINE, MUL_SMALL, FROM_AFFINE, NEG_AFFINE = OPS = range(7)
NAMES = ["add", "add_affine", "dbl", "dbl_affine", "mul_small", "from_affine", "neg_affine"]
N_RANDOM = 3000
MUL_KS = [0, 1, 2, 3, 127, 128, 255, 256, 2**15 - 1, 2**15, 2**31, 2**32 - 1]
ID0 = (0, 0, 0, 0)


def lift(pt, z):
    """the XYZZ form of an affine point under z (None: the all-zero identity)"""
    if pt is None:
        return ID0
    z2 = z * z % P
    z3 = z2 * z % P
    return pt[0] * z2 % P, pt[1] * z3 % P, z2, z3


def affine(pt):
    return (0, 0) if pt is None else pt


def xyzz_dbl(p):
    """dbl-2008-s-1 on integers: the representation of 2P that an XYZZ doubling of P leaves"""
    X, Y, ZZ, ZZZ = p
    U = 2 * Y % P
    V = U * U % P
    W = U * V % P
    S = X * V % P
    M = 3 * X * X % P
    X3 = (M * M - 2 * S) % P
    return X3, (M * (S - X3) - W * Y) % P, V * ZZ % P, W * ZZZ % P


def rows(tuples):
    """canonical Fq integers, one tuple per row -> uint64[n, 6 len(tuple)] of Montgomery limbs"""
    raw = b"".join((v * G.RQ % P).to_bytes(48, "little") for t in tuples for v in t)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(tuples), -1).copy()


def raw_ints(a):
    """uint64[n, 6 c] -> n tuples of c raw (Montgomery) integers"""
    n, c = a.shape[0], a.shape[1] // 6
    raw = np.ascontiguousarray(a).tobytes()
    return [tuple(int.from_bytes(raw[48 * (c * i + j):48 * (c * i + j + 1)], "little") for j in range(c)) for i in range(n)]


def xyzz_is(raw, want):
    """one result of raw Montgomery integers (X, Y, ZZ, ZZZ) against the model's affine point (None: the identity)"""
    if any(v >= P for v in raw):
        return False
    X, Y, ZZ, ZZZ = (v * RINV % P for v in raw)
    if ZZ == 0:
        return want is None
    if want is None or pow(ZZ, 3, P) != ZZZ * ZZZ % P:
        return False
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P) == want


def bad_rows(op, out, want):
    """the first few rows of an operation's output (uint64[n, 24], [n, 12] for NEG_AFFINE) that differ from the model"""
    if len(out) != len(want):
        return ["%d rows for %d" % (len(out), len(want))]
    if op == NEG_AFFINE:
        return [i for i, w in enumerate(want) if out[i].tolist() != G.point_limbs(w)][:5]
    return [i for i, (r, w) in enumerate(zip(raw_ints(out), want)) if not xyzz_is(r, w)][:5]


@functools.lru_cache(maxsize=None)
def points():
    """(the 65 named points, 512 further points of a walk)"""
    rng = random.Random(0x61)
    ks = [1, 2, 3, R - 1, R - 2] + [rng.randrange(1, R) for _ in range(60)]
    return [G.mul(k, G.G) for k in ks], CM.subgroup_walk(512, 0x62)


def _additions(rng, pts, walk, mixed):
    """operand pairs for ADD (mixed: for ADD_AFFINE, whose second operand is affine) with the model's sums"""
    A, B, W = [], [], []
    rz = lambda: rng.randrange(1, P)  # noqa: E731
    zs = [1, 2, P - 1, rz(), rz()]
    second = (lambda pt, z: affine(pt)) if mixed else lift
    fake = lambda: (rz(), rz(), 0, rz())  # noqa: E731  (an identity with stray coordinates)

    def put(a, b, want):
        A.append(a)
        B.append(b)
        W.append(want)

    for i, p in enumerate(pts):
        q, two = pts[(i + 1) % len(pts)], G.add(p, p)
        for za in zs:
            for zb in ([1] if mixed else zs):
                put(lift(p, za), second(q, zb), G.add(p, q))                       # general
                put(lift(p, za), second(p, zb), two)                               # P + P, the same and two different z
                put(lift(p, za), second(G.neg(p), zb), None)                       # P - P
                put(xyzz_dbl(lift(p, za)), second(two, zb), G.add(two, two))       # 2P as a sum + 2P freshly lifted
                put(xyzz_dbl(lift(p, za)), second(G.neg(two), zb), None)
            put(ID0, second(p, za), p)                                             # the identity on either side, both forms
            put(fake(), second(p, za), p)
            put(lift(p, za), second(None, 1), p)
            if not mixed:
                put(lift(p, za), fake(), p)
                put(second(two, za), xyzz_dbl(lift(p, zs[i % 5])), G.add(two, two))
    put(ID0, second(None, 1), None)
    put(fake(), second(None, 1), None)
    if not mixed:
        put(ID0, fake(), None)
        put(fake(), fake(), None)
    for i in range(N_RANDOM):
        p, q = walk[rng.randrange(len(walk))], walk[rng.randrange(len(walk))]
        put(lift(p, rz()), second(q, rz()), G.add(p, q))
    return A, B, W


@functools.lru_cache(maxsize=None)
def corpus():
    """{op: (a, b, k, want)}: operands as uint64 limb rows (b and k None where the operation takes none), want a list of the
    model's affine points"""
    rng = random.Random(0x63)
    pts, walk = points()
    rz = lambda: rng.randrange(1, P)  # noqa: E731
    out = {}
    for op in (ADD, ADD_AFFINE):
        A, B, W = _additions(rng, pts, walk, op == ADD_AFFINE)
        out[op] = (rows(A), rows(B), None, W)
    # doublings: every point under every z, both identities, random lifts
    A = [lift(p, z) for p in pts for z in (1, 2, P - 1, rz())] + [ID0, (rz(), rz(), 0, rz())]
    W = [G.add(p, p) for p in pts for _ in range(4)] + [None, None]
    for _ in range(N_RANDOM):
        p = walk[rng.randrange(len(walk))]
        A.append(lift(p, rz()))
        W.append(G.add(p, p))
    out[DBL] = (rows(A), None, None, W)
    out[DBL_AFFINE] = (rows(pts + walk), None, None, [G.add(p, p) for p in pts + walk])  # (defined for real points only)
    out[FROM_AFFINE] = (rows([affine(p) for p in [None] + pts + walk]), None, None, [None] + pts + walk)
    out[NEG_AFFINE] = (rows([affine(p) for p in [None] + pts + walk]), None, None, [G.neg(p) for p in [None] + pts + walk])
    # k P at the bit edges of k: operands with ZZ != 1, and both identities
    ops = [(p, lift(p, z)) for p in pts[:8] for z in (2, P - 1, rz())] + [(None, ID0), (None, (rz(), rz(), 0, rz()))]
    A = [a for _, a in ops for _ in MUL_KS]
    K = [k for _ in ops for k in MUL_KS]
    W = [G.mul(k, p) for p, _ in ops for k in MUL_KS]
    for i in range(N_RANDOM // 2):
        p, k = walk[rng.randrange(len(walk))], rng.getrandbits(1 + i % 32)
        A.append(lift(p, rz()))
        K.append(k)
        W.append(G.mul(k, p))
    out[MUL_SMALL] = (rows(A), None, np.array(K, dtype=np.uint32), W)
    return out
