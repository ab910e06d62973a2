"""CPU: pg_g1_to_compressed (the library's host code over csrc/fq.hpp's host forms) against the model and the known answers for
G, -G, the identity and random points; and the argument errors.  No GPU needed."""
import ctypes as C
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import g1_model as M  # noqa: E402

G_COMPRESSED = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"


def test_known_answers():
    import plonk_gadgets_amd as pg
    g = pg.G1Affine.generator()
    assert list(g.limbs) == M.point_limbs(M.G)
    assert g.to_compressed().hex() == G_COMPRESSED
    assert pg.G1Affine.identity().to_compressed() == bytes([0xC0]) + bytes(47)
    assert pg.G1Affine.from_ints(*M.neg(M.G)).to_compressed() == M.compressed(M.neg(M.G))
    assert g.to_ints() == M.G and pg.G1Affine.identity().to_ints() is None
    assert g == pg.G1Affine.generator() and g != pg.G1Affine.identity()


def test_random_points_in_one_call():
    from plonk_gadgets_amd import _lib
    lib = _lib.load()
    rng = random.Random(5)
    pts = [M.mul(rng.randrange(1, M.R_FR), M.G) for _ in range(40)] + [None, M.G, M.neg(M.G)]
    arr = (_lib.G1AffineC * len(pts))()
    for i, p in enumerate(pts):
        limbs = M.point_limbs(p)
        for k in range(6):
            arr[i].x[k], arr[i].y[k] = limbs[k], limbs[6 + k]
    out = (C.c_uint8 * (48 * len(pts)))()
    assert lib.pg_g1_to_compressed(arr, len(pts), out) == 0
    got = bytes(out)
    for i, p in enumerate(pts):
        assert got[48 * i:48 * i + 48] == M.compressed(p), i


def test_argument_errors():
    from plonk_gadgets_amd import _lib
    lib = _lib.load()
    out = (C.c_uint8 * 48)()
    assert lib.pg_g1_to_compressed(None, 1, out) == 2
    assert lib.pg_g1_to_compressed(None, 0, None) == 0
    bad = _lib.G1AffineC()
    for k in range(6):
        bad.x[k] = (1 << 64) - 1
    assert lib.pg_g1_to_compressed(C.byref(bad), 1, out) == 2
