"""GPU: every device call issued on a stream that is BEHIND (tests/lagging_stream.py), against the Python-integer models.

The rest of the suite drives the library from the default stream with nothing in flight: the host issues each call long after its
inputs exist on the device.  Here the stream a call is issued on still has a delay of tens of milliseconds in front of it, the true
inputs are copied in BEHIND that delay, and what the buffers hold while the host issues the call is stale -- valid inputs of the
same shape whose answer differs -- so a launch on another stream, scratch shared by two calls on two streams, or a caller's buffer
written on one stream and read on another gives the stale answer (or a sentinel), never a wild address.  Every test asserts that the
delay was still running when its call was issued (event.query() is False: after a call that only enqueues, right before one that
synchronises); none can pass because the stream had caught up.

  A. each entry point, inputs and outputs on the caller's lagging stream;
  B. one engine moving between two streams while its scratch is in use (a row per scratch owner of pg_engine);
  C. a composer made on one stream and used under another, both ways round;
  D. prove and the four verify functions under a lagging stream.

Expected values are the models' (ntt_model, perm_product_model, quotient*_model, opening_model, g1_model, g1_codec_model,
range_gate_model, plonk_verify_model, oracle/pyoracle; for pg_plonk_sides the host routine pg_plonk_sides_host, as in
tests/test_gpu_plonk_sides.py), never a second run of the call."""
import ctypes as C
import functools
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import _lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import g1_codec_model as CM  # noqa: E402
import plonk_sides_corpus as K  # noqa: E402
import g1_model as GM  # noqa: E402
import ntt_model as NM  # noqa: E402
import opening_model as OM  # noqa: E402
import perm_product_model as PM  # noqa: E402
import plonk_verify_model as VM  # noqa: E402
import quotient_blinded_model as BM  # noqa: E402
import quotient_model as QM  # noqa: E402
import quotient_range_model as RM  # noqa: E402
import range_gate_model as GATE  # noqa: E402
from lagging_stream import LATE, TARGET_MS, calibration, lagging, release  # noqa: E402

DEV = "cuda:0"
Q = PM.Q
S = pg.BlsScalar.from_int
ALPHA, BETA, GAMMA = 0x5EED_0A01 ** 7 % Q, 0x5EED_0A02 ** 9 % Q, 0x5EED_0A03 ** 11 % Q
POINT = 0x5EED_0A04 ** 13 % Q
TAU = 0x5EED_0A05 ** 9 % Q
SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def side():
    """the one side stream of sections A, C and D (with the default stream and, in B, a third: at most three alive in a test)"""
    return torch.cuda.Stream()


@pytest.fixture(scope="module", autouse=True)
def delay(side):
    """the delay, measured on the idle side stream; its 1 GiB tensor is given back when the module is through"""
    cal = calibration(side)
    print("\nlagging_stream: %.3f ms per pass, %d passes, a delay of %.1f ms" % (cal["ms_per_pass"], cal["passes"], cal["delay_ms"]))
    assert cal["delay_ms"] >= TARGET_MS
    yield cal
    release()


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def host(t):
    return t.cpu().numpy().view(np.uint64)


def ints(t):
    return PM.ints_of(host(t))


def dev_limbs(xs):
    """canonical ints -> int64[n, 4] Montgomery limbs on the device"""
    return torch.from_numpy(PM.limbs_of(xs).view(np.int64)).to(DEV)


def dev_np(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def field_ints(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(Q) for _ in range(n)]


def cloned(x):
    """the device tensors among a call's results, copied on the current stream without synchronising"""
    if isinstance(x, torch.Tensor):
        return x.clone() if x.is_cuda else x
    if isinstance(x, (tuple, list)):
        return type(x)(cloned(v) for v in x)
    if isinstance(x, dict):
        return {k: cloned(v) for k, v in x.items()}
    return x


def behind(side, bufs, call, enqueues, warm=True):
    """call() under the lagging stream `side`.  bufs: (buffer, stale, true) device tensors: while the host issues the call the
    buffers hold the stale contents, the true ones are copied in on `side` behind the delay.  With warm, the call runs twice before
    on the stale contents -- on the default stream (the engine's scratch grows there) and on `side` (torch's allocator gets that
    stream's blocks) -- so that the run that counts allocates nothing.  enqueues: the call only enqueues (its device results are
    then copied on `side`, still without a synchronisation, and the delay must outlast all of that); otherwise it synchronises the
    host, and the delay must still be running right before it.  Returns the call's result."""
    def stale():
        for b, s, _ in bufs:
            b.copy_(s)
        torch.cuda.synchronize()
    if warm:
        stale()
        call()
        torch.cuda.synchronize()
        stale()
        with torch.cuda.stream(side):
            out = cloned(call())
        torch.cuda.synchronize()
        del out
    stale()
    with torch.cuda.stream(side):
        ev = lagging(side)
        for b, _, t in bufs:
            b.copy_(t)
        if enqueues:
            out = cloned(call())
        else:
            assert not ev.query(), LATE
            out = call()
        if enqueues:
            assert not ev.query(), LATE
    torch.cuda.synchronize()
    return out


# ---- A. each entry point on the caller's lagging stream ---------------------------------------------------------------------
NTT_M, NTT_COLS, NTT_PAD = 12, 3, 5  # 2^12 points: one strided pass, the tile pass and the reversal; three columns at a stride


@functools.lru_cache(maxsize=None)
def ntt_case():
    n = 1 << NTT_M
    true = [field_ints(n, 100 + j) for j in range(NTT_COLS)]
    stale = [field_ints(n, 200 + j) for j in range(NTT_COLS)]
    return true, stale


@functools.lru_cache(maxsize=None)
def ntt_expected(kind):
    true, stale = ntt_case()
    return [NM.KINDS[kind](c) for c in true], [NM.KINDS[kind](c) for c in stale]


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("kind", list(NM.KINDS))
def test_ntt(engine, side, kind, inplace):
    n = 1 << NTT_M
    true, stale = ntt_case()
    exp, exp_stale = ntt_expected(kind)
    assert all(a != b for a, b in zip(exp, exp_stale))
    buf = torch.full((NTT_COLS, n + NTT_PAD, 4), SENTINEL, dtype=torch.int64, device=DEV)
    t_true, t_stale = torch.stack([dev_limbs(c) for c in true]), torch.stack([dev_limbs(c) for c in stale])
    view = buf[:, :n]
    got = behind(side, [(view, t_stale, t_true)], lambda: getattr(engine, kind)(view, inplace=inplace), enqueues=True)
    for j in range(NTT_COLS):
        assert np.array_equal(host(got[j]), PM.limbs_of(exp[j])), (kind, j)
    assert bool((buf[:, n:] == SENTINEL).all())
    if not inplace:
        assert torch.equal(view, t_true)


PP_N, PP_VALUES = 1 << 12, 3000


@functools.lru_cache(maxsize=None)
def sigma_case():
    """(true, stale): a random permutation of the 4 * PP_N positions, and the identity"""
    rng = np.random.default_rng(31)
    return rng.permutation(4 * PP_N).astype(np.uint64).reshape(4, PP_N), np.arange(4 * PP_N, dtype=np.uint64).reshape(4, PP_N)


def test_sigma_evaluations(engine, side):
    true, stale = sigma_case()
    omega = PM.omega_of(12)
    exp, exp_stale = PM.sigma_evaluations(true, PP_N, omega), PM.sigma_evaluations(stale, PP_N, omega)
    assert exp != exp_stale
    buf = torch.empty((4, PP_N), dtype=torch.int64, device=DEV)
    # (it synchronises: the verdict on sigma's entries comes back from the device)
    got = behind(side, [(buf, dev_np(stale), dev_np(true))], lambda: engine.sigma_evaluations(buf), enqueues=False)
    assert np.array_equal(host(got).reshape(4 * PP_N, 4), PM.limbs_of([x for j in range(4) for x in exp[j]]))


def test_permutation_product(engine, side):
    sig_true, sig_stale = sigma_case()
    w_true = [field_ints(PP_VALUES, 40 + j) for j in range(4)]
    w_stale = [field_ints(PP_VALUES, 50 + j) for j in range(4)]
    omega = PM.omega_of(12)
    ez, ewrap = PM.grand_product(w_true, sig_true, PP_N, BETA, GAMMA, omega)
    sz, swrap = PM.grand_product(w_stale, sig_stale, PP_N, BETA, GAMMA, omega)
    assert ez != sz and ewrap != swrap
    sigma = torch.empty((4, PP_N), dtype=torch.int64, device=DEV)
    wires = [torch.empty((PP_VALUES, 4), dtype=torch.int64, device=DEV) for _ in range(4)]
    z_out = torch.empty((PP_N + 3, 4), dtype=torch.int64, device=DEV)
    sentinel = torch.full_like(z_out, SENTINEL)
    bufs = [(sigma, dev_np(sig_stale), dev_np(sig_true)), (z_out, sentinel, sentinel)]
    bufs += [(wires[j], dev_limbs(w_stale[j]), dev_limbs(w_true[j])) for j in range(4)]
    z, wrap = behind(side, bufs, lambda: engine.permutation_product(wires, sigma, S(BETA), S(GAMMA), z_out=z_out), enqueues=False)
    assert z.data_ptr() == z_out.data_ptr() and wrap.to_int() == ewrap
    assert np.array_equal(host(z[:PP_N]), PM.limbs_of(ez))
    assert bool((z[PP_N:] == SENTINEL).all())


QUOT_M = 9  # n = 512: every transform of the 4n points is a strided pass, a tile pass and a reversal


def quotient_inputs(seed, blinded):
    """18 columns of n + 4 rows (tests/test_gpu_quotient_range.py): blinded, the wires use n + 2 of them and z n + 3, the rest n"""
    n = 1 << QUOT_M
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 2**64, size=(18, n + 4, 4), dtype=np.uint64)
    raw[..., 3] %= np.uint64(0x73EDA753299D7D48)
    return torch.from_numpy(raw.view(np.int64)).to(DEV)


def quotient_polys(x, blinded, with_range):
    n = 1 << QUOT_M
    rows = ([n + 2] * 4 + [n + 3] if blinded else [n] * 5) + [n] * 13
    polys = {"wires": [x[j, :rows[j]] for j in range(4)], "z": x[4, :rows[4]], "sigmas": [x[5 + j, :n] for j in range(4)],
             "pi": x[16, :n], "selectors": {name: x[9 + i, :n] for i, name in enumerate(QM.SELECTORS)}}
    if with_range:
        polys["q_range"] = x[17, :n]
    return polys


def quotient_ints(polys):
    out = {name: ints(polys["wires"][j]) for j, name in enumerate(BM.WIRES)}
    out["z"] = ints(polys["z"])
    for j in range(4):
        out["s%d" % (j + 1)] = ints(polys["sigmas"][j])
    for name in QM.SELECTORS:
        out[name] = ints(polys["selectors"][name])
    out["pi"] = ints(polys["pi"])
    if "q_range" in polys:
        out["q_range"] = ints(polys["q_range"])
    return out


@pytest.mark.parametrize("which", ["quotient", "quotient_blinded", "quotient_with_q_range"])
def test_quotients(engine, side, which):
    n = 1 << QUOT_M
    blinded, with_range = which == "quotient_blinded", which == "quotient_with_q_range"
    model = BM.quotient_blinded if blinded else RM.quotient if with_range else QM.quotient
    t_true, t_stale = quotient_inputs(61, blinded), quotient_inputs(62, blinded)
    exp = model(quotient_ints(quotient_polys(t_true, blinded, with_range)), ALPHA, BETA, GAMMA)
    exp_stale = model(quotient_ints(quotient_polys(t_stale, blinded, with_range)), ALPHA, BETA, GAMMA)
    assert exp != exp_stale
    x = torch.empty_like(t_true)
    polys = quotient_polys(x, blinded, with_range)
    scratch = torch.empty((8, n, 4), dtype=torch.int64, device=DEV)
    fn = engine.quotient_blinded if blinded else engine.quotient
    got = behind(side, [(x, t_stale, t_true)],
                 lambda: fn(**polys, alpha=S(ALPHA), beta=S(BETA), gamma=S(GAMMA), scratch=scratch), enqueues=True)
    assert np.array_equal(host(got).reshape(-1, 4), PM.limbs_of(exp)), which
    assert torch.equal(x, t_true)


def test_blind(engine, side):
    """Engine.blind goes through the host for the few rows it changes: a wire (two blinders) and z (three)"""
    n = 1 << 10
    for blinders, seed in (([5, 7], 71), ([11, 13, 17], 72)):
        c = len(blinders)
        true, stale = field_ints(n, seed) + [0] * 8, field_ints(n, seed + 100) + [0] * 8
        exp, exp_stale = BM.blind(true[:n], n, blinders), BM.blind(stale[:n], n, blinders)
        assert exp[:c] != exp_stale[:c]
        buf = torch.empty((n + 8, 4), dtype=torch.int64, device=DEV)
        got = behind(side, [(buf, dev_limbs(stale), dev_limbs(true))], lambda: engine.blind(buf, n, blinders), enqueues=False)
        assert got.data_ptr() == buf.data_ptr()
        assert ints(buf) == list(exp) + [0] * (n + 8 - len(exp))


def test_evaluate(engine, side):
    n, cols, pad = 3001, 3, 7  # not a power of two; three columns at a stride
    true, stale = [field_ints(n, 80 + j) for j in range(cols)], [field_ints(n, 90 + j) for j in range(cols)]
    exp, exp_stale = [OM.horner(c, POINT) for c in true], [OM.horner(c, POINT) for c in stale]
    assert all(a != b for a, b in zip(exp, exp_stale))
    buf = torch.full((cols, n + pad, 4), SENTINEL, dtype=torch.int64, device=DEV)
    view = buf[:, :n]
    t_true, t_stale = torch.stack([dev_limbs(c) for c in true]), torch.stack([dev_limbs(c) for c in stale])
    got = behind(side, [(view, t_stale, t_true)], lambda: engine.evaluate(view, POINT), enqueues=False)
    assert [v.to_int() for v in got] == exp


OPEN_N, OPEN_MU = 5000, [3, Q - 1, 0x5EED_0A06 ** 5 % Q]  # more than two tiles of 2048 coefficients, the last one short


@functools.lru_cache(maxsize=None)
def open_case():
    true, stale = [field_ints(OPEN_N, 110 + j) for j in range(3)], [field_ints(OPEN_N, 120 + j) for j in range(3)]
    return true, stale


def test_open(engine, side):
    true, stale = open_case()
    (eq, erem), (sq, srem) = OM.open_(true, OPEN_MU, POINT), OM.open_(stale, OPEN_MU, POINT)
    assert eq != sq and erem != srem
    buf = torch.empty((3, OPEN_N, 4), dtype=torch.int64, device=DEV)
    t_true, t_stale = torch.stack([dev_limbs(c) for c in true]), torch.stack([dev_limbs(c) for c in stale])
    w, v = behind(side, [(buf, t_stale, t_true)], lambda: engine.open(buf, OPEN_MU, POINT), enqueues=False)
    assert v.to_int() == erem and ints(w) == eq


def test_combine(engine, side):
    true, stale = open_case()
    exp, exp_stale = OM.combine(true, OPEN_MU), OM.combine(stale, OPEN_MU)
    assert exp != exp_stale
    buf = torch.empty((3, OPEN_N, 4), dtype=torch.int64, device=DEV)
    t_true, t_stale = torch.stack([dev_limbs(c) for c in true]), torch.stack([dev_limbs(c) for c in stale])
    got = behind(side, [(buf, t_stale, t_true)], lambda: engine.combine(buf, OPEN_MU), enqueues=True)
    assert ints(got) == exp


MSM_N = 300


@functools.lru_cache(maxsize=None)
def basis():
    """2 * MSM_N known multiples k_i G: the first MSM_N are the true bases, the others the stale ones"""
    rng = random.Random(0xB45E)
    ks = [rng.randrange(1, GM.R_FR) for _ in range(2 * MSM_N)]
    return ks, [GM.mul(k, GM.G) for k in ks]


def points_tensor(pts):
    return pg.g1.points_tensor([pg.G1Affine(GM.point_limbs(p)) for p in pts], DEV)


def sum_of(scalars, ks):
    return GM.point_limbs(GM.mul(sum(s * k for s, k in zip(scalars, ks)) % GM.R_FR, GM.G))


def msm_buffers():
    ks, pts = basis()
    cols_true = [field_ints(MSM_N, 130), field_ints(MSM_N, 131)]
    cols_stale = [field_ints(MSM_N, 132), field_ints(MSM_N, 133)]
    bases = torch.empty((MSM_N, 12), dtype=torch.int64, device=DEV)
    scalars = torch.empty((2, MSM_N, 4), dtype=torch.int64, device=DEV)
    bufs = [(bases, points_tensor(pts[MSM_N:]), points_tensor(pts[:MSM_N])),
            (scalars, torch.stack([dev_limbs(c) for c in cols_stale]), torch.stack([dev_limbs(c) for c in cols_true]))]
    return ks, cols_true, cols_stale, bases, scalars, bufs


def test_msm(engine, side):
    ks, cols_true, cols_stale, bases, scalars, bufs = msm_buffers()
    exp = [sum_of(c, ks[:MSM_N]) for c in cols_true]
    assert exp != [sum_of(c, ks[MSM_N:]) for c in cols_stale]
    got = behind(side, bufs, lambda: engine.msm(bases, scalars), enqueues=False)  # (the points come back to the host)
    assert [list(p.limbs) for p in got] == exp


def test_commit(engine, side):
    """CommitKey.commit: the key's powers and the polynomials both arrive on the lagging stream"""
    ks, cols_true, cols_stale, bases, scalars, bufs = msm_buffers()
    exp = [sum_of(c, ks[:MSM_N]) for c in cols_true]
    assert exp != [sum_of(c, ks[MSM_N:]) for c in cols_stale]
    ck = pg.CommitKey(engine, bases)
    got = behind(side, bufs, lambda: ck.commit(scalars), enqueues=False)
    assert [list(p.limbs) for p in got] == exp
    one = behind(side, bufs, lambda: ck.commit(scalars[1]), enqueues=False)
    assert list(one.limbs) == exp[1]


def test_msm_segmented(engine, side):
    ks, cols_true, cols_stale, bases, scalars, bufs = msm_buffers()
    offsets = [0, 23, 23, 150, 299, 300]  # an empty segment among them

    def sums(cols, kk):
        return [[sum_of(c[a:b], kk[a:b]) if b > a else [0] * 12 for c in cols] for a, b in zip(offsets, offsets[1:])]
    exp = sums(cols_true, ks[:MSM_N])
    assert exp != sums(cols_stale, ks[MSM_N:])
    got = behind(side, bufs, lambda: engine.msm_segmented(bases, scalars, offsets), enqueues=True)
    assert got.shape == (5, 2, 12)
    assert host(got).tolist() == exp


def test_srs_setup(engine, side):
    """pg_srs_setup into the caller's buffer, which gets its sentinel ON the lagging stream: a launch that went elsewhere would
    have run before the fill"""
    n = 200
    exp = [GM.point_limbs(GM.mul(pow(TAU, i, GM.R_FR), GM.G)) for i in range(n)]
    out = torch.empty((n, 12), dtype=torch.int64, device=DEV)
    sentinel = torch.full_like(out, SENTINEL)

    def call():
        st = engine._lib.pg_srs_setup(engine._h, C.byref(S(TAU).c), None, n, out.data_ptr(), engine._stream())
        assert st == 0, engine._lib.pg_last_error()
        return out
    got = behind(side, [(out, sentinel, sentinel)], call, enqueues=True)
    assert host(got).tolist() == exp
    # and CommitKey.setup, whose buffer is its own
    ck = behind(side, [], lambda: pg.CommitKey.setup(engine, n - 1, S(TAU)).powers, enqueues=True)
    assert host(ck).tolist() == exp


CODEC_N = 300


@functools.lru_cache(maxsize=None)
def codec_case():
    """(true, stale) lists of CODEC_N curve points: multiples of G, every seventh (true) or fifth (stale) one a point of the
    curve outside the subgroup"""
    ks, pts = basis()
    rng = random.Random(0xC0DEC)
    outside = [CM.curve_point_from_x(rng) for _ in range(8)]
    assert not any(CM.in_subgroup(p) for p in outside)
    true = [outside[i % 8] if i % 7 == 3 else pts[i] for i in range(CODEC_N)]
    stale = [outside[(i + 1) % 8] if i % 5 == 2 else pts[CODEC_N + i] for i in range(CODEC_N)]
    return true, stale


def statuses(pts):
    return [0 if CM.in_subgroup(p) else 3 for p in pts]  # PG_G1_OK, PG_G1_NOT_IN_SUBGROUP


def test_g1_decompress(engine, side):
    true, stale = codec_case()
    enc = lambda pts: torch.frombuffer(bytearray(b"".join(GM.compressed(p) for p in pts)), dtype=torch.uint8).to(DEV)
    assert statuses(true) != statuses(stale)
    data = torch.empty((48 * CODEC_N,), dtype=torch.uint8, device=DEV)
    points, status = behind(side, [(data, enc(stale), enc(true))], lambda: engine.g1_decompress(data), enqueues=True)
    assert status.cpu().tolist() == statuses(true)
    exp = [GM.point_limbs(p) if s == 0 else [0] * 12 for p, s in zip(true, statuses(true))]  # a rejected point is the identity
    assert host(points).tolist() == exp


def test_g1_check_and_compress(engine, side):
    true, stale = codec_case()
    assert statuses(true) != statuses(stale)
    pts = torch.empty((CODEC_N, 12), dtype=torch.int64, device=DEV)
    bufs = [(pts, points_tensor(stale), points_tensor(true))]
    assert behind(side, bufs, lambda: engine.g1_check(pts), enqueues=True).cpu().tolist() == statuses(true)
    got = behind(side, bufs, lambda: engine.g1_compress(pts), enqueues=True)
    assert got.cpu().numpy().tobytes() == b"".join(GM.compressed(p) for p in true)


def test_commit_key_from_bytes_in_chunks(engine, side):
    """CommitKey.from_bytes with a chunk smaller than the key: the pinned buffer is filled again while a decode is pending, all of
    it on the lagging stream"""
    ks, pts = basis()
    data = b"".join(GM.compressed(p) for p in pts[:CODEC_N])
    pg.CommitKey.from_bytes(engine, data, chunk=64)  # (warm: default stream)
    with torch.cuda.stream(side):
        pg.CommitKey.from_bytes(engine, data, chunk=64)
        torch.cuda.synchronize()
        ev = lagging(side)
        assert not ev.query(), LATE
        ck = pg.CommitKey.from_bytes(engine, data, chunk=64)
        powers = ck.powers.clone()
    torch.cuda.synchronize()
    assert host(powers).tolist() == [GM.point_limbs(p) for p in pts[:CODEC_N]]


@functools.lru_cache(maxsize=None)
def sides_key():
    return K.make_key(1 << 12, 0x51DE).record(K.Ok, b"plonk")


@functools.lru_cache(maxsize=None)
def sides_batch(n, every, at, seed):
    """the bytes of n synthetic proofs (tests/plonk_sides_corpus.py); proof i with i % every == at carries a commitment that is
    rejected -- the four classes in turn, at commitments that move with i"""
    base = [K.make_proof(seed + i).to_bytes() for i in range(3)]
    rejected = [enc for enc, _ in K.rejected_encodings().values()]
    proofs = []
    for i in range(n):
        p = base[i % 3]
        if i % every == at:
            p = K.with_commitment(p, (5 * i) % 11, rejected[(i // every) % len(rejected)])
        proofs.append(p)
    return b"".join(proofs)


def host_sides(data):
    """pg_plonk_sides_host's four outputs for proofs under sides_key(), as bytes"""
    st, bases, scalars, status, where = K.host_sides(data, [sides_key()])
    assert st == 0
    return bases, scalars, status, where


def device_sides(out):
    bases, scalars, status, where = out
    return tuple(t.cpu().numpy().tobytes() for t in (bases, scalars, status, where))


def proofs_on_device(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)


def test_plonk_sides(engine, side):
    """100 proofs (two workgroups), every third rejected at one commitment; stale: other proofs, every fourth rejected"""
    true, stale = sides_batch(100, 3, 1, 0x700), sides_batch(100, 4, 2, 0x710)
    exp, exp_stale = host_sides(true), host_sides(stale)
    assert all(a != b for a, b in zip(exp, exp_stale)) and set(exp[2]) == {0, 1, 2, 3}
    keys = proofs_on_device(sides_key())
    buf = torch.empty((len(true),), dtype=torch.uint8, device=DEV)
    got = behind(side, [(buf, proofs_on_device(stale), proofs_on_device(true))], lambda: engine.plonk_sides(buf, keys), enqueues=True)
    assert device_sides(got) == exp


def canonical_rows(values):
    return np.array([[(x >> (64 * i)) & (2**64 - 1) for i in range(4)] for x in values], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def encodings_case():
    """(true, stale) canonical encodings, 700 each (three workgroups): 9 of the true ones and 4 of the stale ones are not below q"""
    true, stale = field_ints(700, 140), field_ints(700, 141)
    for i in range(9):
        true[70 * i + 5] = Q + i
    for i in range(4):
        stale[100 * i + 1] = 2**256 - 1 - i
    return true, stale


def test_scalars_from_and_to_canonical(engine, side):
    true, stale = encodings_case()
    raw = torch.empty((700, 4), dtype=torch.int64, device=DEV)
    bufs = [(raw, dev_np(canonical_rows(stale)), dev_np(canonical_rows(true)))]
    out, bad, nbad = behind(side, bufs, lambda: engine.scalars_from_canonical(raw), enqueues=False)
    assert nbad == 9 and bad.cpu().tolist() == [int(x >= Q) for x in true]
    assert np.array_equal(host(out), PM.limbs_of([x if x < Q else 0 for x in true]))
    good_true, good_stale = [x % Q for x in true], [x % Q for x in stale]
    mont = torch.empty((700, 4), dtype=torch.int64, device=DEV)
    got = behind(side, [(mont, dev_limbs(good_stale), dev_limbs(good_true))], lambda: engine.scalars_to_canonical(mont), enqueues=True)
    assert np.array_equal(host(got), canonical_rows(good_true))


# ---- B. one engine moving between streams while its scratch is in use ------------------------------------------------------
def functions_that_only_enqueue():
    """the C entry points whose comment in include/plonk_gadgets_hip.h says that they only enqueue: every declaration with a
    `stream` argument that follows such a comment, up to the next comment that starts a line"""
    text = open(os.path.join(ROOT, "include", "plonk_gadgets_hip.h")).read()
    names = []
    for m in re.finditer(r"^/\*(.*?)\*/(.*?)(?=^/\*|\Z)", text, re.S | re.M):
        comment, code = m.group(1), m.group(2)
        if re.search(r"only\s+enqueues?\b|Enqueues\s+only", comment):
            names += re.findall(r"pg_status\s+(pg_\w+)\s*\([^;]*void \*stream\)", code)
    return sorted(names)


ONLY_ENQUEUE = ["pg_g1_check", "pg_g1_compress", "pg_g1_decompress", "pg_msm", "pg_msm_segmented", "pg_ntt", "pg_pairing_check",
                "pg_pairing_gt", "pg_plonk_sides", "pg_poly_combine", "pg_poly_evaluate", "pg_poly_open", "pg_quotient",
                "pg_quotient_blinded", "pg_srs_setup"]

# scratch owner of pg_engine -> the call X of its row (a member of ONLY_ENQUEUE, or None with the reason):
OWNERS = {
    "d_ntt": "pg_ntt",
    "d_pp": None,            # pg_sigma_evaluations and pg_permutation_product both synchronise: the device reports bad entries
    "d_quot": "pg_quotient",
    "d_eval": "pg_poly_evaluate",
    "d_open": "pg_poly_open",
    "d_msm": "pg_msm",
    "d_msm_small": "pg_msm_segmented",
    "d_sides": "pg_plonk_sides",
    "pairing": None,         # pg_pairing_check keeps no device memory (the header says so): nothing to share
    "d_err_count": None,     # the plan calls are not in the header's list: their asynchronous forms are the X of their own row below
}


def test_the_calls_that_only_enqueue_are_the_headers():
    assert functions_that_only_enqueue() == ONLY_ENQUEUE
    assert all(x is None or x in ONLY_ENQUEUE for x in OWNERS.values())


@pytest.fixture(scope="module")
def second():
    """the third stream of section B (beside the default stream and `side`)"""
    return torch.cuda.Stream()


def two_streams(s1, s2, x_call, y_call, y_waits=False):
    """X on the lagging stream s1; with no synchronisation, Y on another stream s2 that is released by the end of s1's delay --
    so that, were nothing to order them, X and Y would run side by side on the scratch they share.  Both calls run before on
    the default stream (the engine's scratch grows there) and on their own (torch's allocator gets that stream's blocks).
    y_waits: Y makes the host wait (it synchronises its stream, or waits for X's copy out of a pinned buffer they share), so the
    delay is checked to be running right before Y and not after it.  Returns (X's, Y's) results."""
    for s, calls in ((torch.cuda.current_stream(), (x_call, y_call)), (s1, (x_call,)), (s2, (y_call,))):
        with torch.cuda.stream(s):
            for c in calls:
                cloned(c())
        torch.cuda.synchronize()
    ev = lagging(s1)
    s2.wait_event(ev)
    with torch.cuda.stream(s1):
        x = cloned(x_call())
    with torch.cuda.stream(s2):
        if y_waits:
            assert not ev.query(), LATE
        y = cloned(y_call())
    assert y_waits or not ev.query(), LATE
    torch.cuda.synchronize()
    return x, y


def test_d_ntt_row(engine, side, second):
    """X: 24 columns of 2^12 points; Y: transforms of 2^11 and 2^10 points, whose tables of other omegas lie where X's do"""
    cx = [field_ints(1 << 12, 300 + j) for j in range(2)]
    cy = [field_ints(1 << 11, 310), field_ints(1 << 10, 311)]
    x_in = torch.stack([dev_limbs(cx[j % 2]) for j in range(24)])
    y_in = [dev_limbs(c) for c in cy]
    x_call = lambda: engine.coset_fft(x_in)
    y_call = lambda: [engine.ifft(y_in[0]), engine.coset_ifft(y_in[1]), engine.fft(y_in[0]), engine.coset_fft(y_in[1])]
    x, y = two_streams(side, second, x_call, y_call)
    exp = [NM.coset_fft(c) for c in cx]
    for j in range(24):
        assert np.array_equal(host(x[j]), PM.limbs_of(exp[j % 2])), j
    for got, want in zip(y, (NM.ifft(cy[0]), NM.coset_ifft(cy[1]), NM.fft(cy[0]), NM.coset_fft(cy[1]))):
        assert np.array_equal(host(got), PM.limbs_of(want))


def quotient_of(engine, x, m):
    n = 1 << m
    polys = {"wires": x[0:4], "z": x[4], "sigmas": x[5:9], "pi": x[16], "selectors": {name: x[9 + i] for i, name in enumerate(QM.SELECTORS)}}
    exp_in = {name: ints(x[i]) for i, name in enumerate(("a", "b", "c", "d", "z", "s1", "s2", "s3", "s4"))}
    exp_in.update({name: ints(x[9 + i]) for i, name in enumerate(QM.SELECTORS)}, pi=ints(x[16]))
    scratch = torch.empty((8, n, 4), dtype=torch.int64, device=DEV)
    return (lambda: engine.quotient(**polys, alpha=S(ALPHA), beta=S(BETA), gamma=S(GAMMA), scratch=scratch)), exp_in


def random_columns(cols, n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 2**64, size=(cols, n, 4), dtype=np.uint64)
    raw[..., 3] %= np.uint64(0x73EDA753299D7D48)
    return torch.from_numpy(raw.view(np.int64)).to(DEV)


def test_d_quot_row(engine, side, second):
    """X: the quotient at n = 2^9; Y: at n = 2^8 -- the table of the chunk's points (and pg_ntt's tables) of another domain"""
    x_call, x_in = quotient_of(engine, random_columns(18, 1 << 9, 320), 9)
    y_call, y_in = quotient_of(engine, random_columns(18, 1 << 8, 321), 8)
    x, y = two_streams(side, second, x_call, y_call)
    assert np.array_equal(host(x).reshape(-1, 4), PM.limbs_of(QM.quotient(x_in, ALPHA, BETA, GAMMA)))
    assert np.array_equal(host(y).reshape(-1, 4), PM.limbs_of(QM.quotient(y_in, ALPHA, BETA, GAMMA)))


def raw_evaluate(engine, polys, point):
    """pg_poly_evaluate itself (Engine.evaluate brings the values to the host, which synchronises)"""
    cols, n = polys.shape[0], polys.shape[1]
    out = torch.empty((cols, 4), dtype=torch.int64, device=DEV)
    st = engine._lib.pg_poly_evaluate(engine._h, polys.data_ptr(), cols, n, n, C.byref(S(point).c), out.data_ptr(), engine._stream())
    assert st == 0, engine._lib.pg_last_error()
    return out


def test_d_eval_row(engine, side, second):
    """X: three columns of 40 000 coefficients at one point; Y: one of 20 001 at another -- other power tables, other partial sums"""
    cx, cy = [field_ints(40_000, 330 + j) for j in range(3)], [field_ints(20_001, 335)]
    x_in, y_in = torch.stack([dev_limbs(c) for c in cx]), torch.stack([dev_limbs(c) for c in cy])
    other = 0x5EED_0A07 ** 11 % Q
    x_call, y_call = (lambda: raw_evaluate(engine, x_in, POINT)), (lambda: raw_evaluate(engine, y_in, other))
    x, y = two_streams(side, second, x_call, y_call)
    assert ints(x) == [OM.horner(c, POINT) for c in cx]
    assert ints(y) == [OM.horner(c, other) for c in cy]


def raw_open(engine, cols, mu, point):
    """pg_poly_open itself (Engine.open reads the value back, which synchronises)"""
    n = cols.shape[1]
    ptrs = (C.c_void_p * cols.shape[0])(*[cols[j].data_ptr() for j in range(cols.shape[0])])
    ws = (_lib.Scalar * cols.shape[0])(*[S(m).c for m in mu])
    w = torch.empty((n, 4), dtype=torch.int64, device=DEV)
    v = torch.empty((1, 4), dtype=torch.int64, device=DEV)
    st = engine._lib.pg_poly_open(engine._h, ptrs, ws, cols.shape[0], n, C.byref(S(point).c), w.data_ptr(), v.data_ptr(), engine._stream())
    assert st == 0, engine._lib.pg_last_error()
    return w, v


def test_d_open_row(engine, side, second):
    """X: an opening over 20 000 coefficients (ten tiles); Y: over 4 097 at another point -- other tile totals and carries"""
    cx, cy = [field_ints(20_000, 340 + j) for j in range(2)], [field_ints(4097, 345)]
    x_in, y_in = torch.stack([dev_limbs(c) for c in cx]), torch.stack([dev_limbs(c) for c in cy])
    other = 0x5EED_0A08 ** 11 % Q
    x_call, y_call = (lambda: raw_open(engine, x_in, [1, 5], POINT)), (lambda: raw_open(engine, y_in, [7], other))
    (xw, xv), (yw, yv) = two_streams(side, second, x_call, y_call)
    eq, erem = OM.open_(cx, [1, 5], POINT)
    assert ints(xw) == eq and ints(xv) == [erem]
    eq, erem = OM.open_(cy, [7], other)
    assert ints(yw) == eq and ints(yv) == [erem]


def raw_msm(engine, bases, scalars):
    """pg_msm itself (Engine.msm brings the points to the host, which synchronises)"""
    out = torch.empty((1, 12), dtype=torch.int64, device=DEV)
    st = engine._lib.pg_msm(engine._h, bases.data_ptr(), scalars.data_ptr(), scalars.shape[0], 1, scalars.shape[0], out.data_ptr(),
                            engine._stream())
    assert st == 0, engine._lib.pg_last_error()
    return out


def test_d_msm_and_d_msm_small_rows(engine, side, second):
    """X: a sum over 300 points; Y: over 120 other points with other scalars -- other sort keys, buckets and window sums (pg_msm),
    other products, sums and segment offsets (pg_msm_segmented)"""
    ks, pts = basis()
    sx, sy = field_ints(300, 350), field_ints(120, 351)
    bx, by = points_tensor(pts[:300]), points_tensor(pts[300:420])
    tx, ty = dev_limbs(sx), dev_limbs(sy)
    ex, ey = sum_of(sx, ks[:300]), sum_of(sy, ks[300:420])
    x_call, y_call = (lambda: raw_msm(engine, bx, tx)), (lambda: raw_msm(engine, by, ty))
    x, y = two_streams(side, second, x_call, y_call)
    assert host(x).tolist() == [ex] and host(y).tolist() == [ey]
    x_call, y_call = (lambda: engine.msm_segmented(bx, tx, [0, 300])), (lambda: engine.msm_segmented(by, ty, [0, 50, 120]))
    # (Y stages its offsets in the pinned buffer X's are still to be copied out of: the host waits for that copy)
    x, y = two_streams(side, second, x_call, y_call, y_waits=True)
    assert host(x).reshape(-1, 12).tolist() == [ex]
    assert host(y).reshape(-1, 12).tolist() == [sum_of(sy[:50], ks[300:350]), sum_of(sy[50:], ks[350:420])]


def test_d_sides_row(engine, side, second):
    """X: 300 proofs, every third with a rejected commitment; Y: 37 and then 64 other proofs, rejected at other places -- other
    decode statuses of the commitments where X's lie.  Bases, scalars, status and where are pg_plonk_sides_host's"""
    dx, dy = sides_batch(300, 3, 1, 0x720), [sides_batch(37, 3, 0, 0x730), sides_batch(64, 2, 0, 0x740)]
    keys = proofs_on_device(sides_key())
    tx, ty = proofs_on_device(dx), [proofs_on_device(d) for d in dy]
    x_call, y_call = (lambda: engine.plonk_sides(tx, keys)), (lambda: [engine.plonk_sides(t, keys) for t in ty])
    x, y = two_streams(side, second, x_call, y_call)
    ex = host_sides(dx)
    assert set(ex[2]) == {0, 1, 2, 3} and ex[2][:37] != host_sides(dy[0])[2]
    assert device_sides(x) == ex
    for got, d in zip(y, dy):
        assert device_sides(got) == host_sides(d)


def test_d_err_count_row(engine, side, second):
    """X: the asynchronous plan of the fused mix over 2^21 + 3000 items, 37 of them zero -- more blocks than one launch plans, so the
    count gathers in e->d_err_count during one kernel and is read by the next; Y: scalars_from_canonical of 700 encodings, 9 of
    them bad, which zeroes, counts in and reads the same word.  X's totals come through the pinned plan result, Y's count
    through a word of its own"""
    batch = (1 << 21) + 3000
    v = synth.random_scalars(batch, seed=360)
    v[(v == 0).all(axis=1)] = synth.mont(1)
    zeros = list(range(11, batch, batch // 37))[:37]
    v[zeros] = 0
    tv = dev_np(v)
    _, roff, voff = engine.ragged_buffers(batch)
    err = torch.zeros((batch,), dtype=torch.uint8, device=DEV)
    true, _ = encodings_case()
    raw = dev_np(canonical_rows(true))
    x_call = lambda: engine.scalar_mix_plan_async(tv, roff, voff, err)
    y_call = lambda: engine.scalars_from_canonical(raw)
    _, (out, bad, nbad) = two_streams(side, second, x_call, y_call, y_waits=True)  # (Y synchronises its stream)
    lay, nerr = engine.plan_result()
    assert nbad == 9 and int(bad.sum()) == 9
    assert nerr == 37 and int(err.sum()) == 37
    assert lay.n_gates == 10 * batch - 2 * 37 and lay.n_vars == 15 * batch - 2 * 37
    assert np.array_equal(host(out), PM.limbs_of([x if x < Q else 0 for x in true]))


# ---- C. a composer made on one stream, used under another ------------------------------------------------------------------
def mixed_circuit_inputs():
    """the witnesses of the circuit of section C, true and stale (valid witnesses of the same shapes, other values)"""
    import bench
    def one(seed):
        mr, wt = bench.c4_inputs(6, seed=seed)
        v, y, s, a, b = bench.mix_inputs(9, seed=seed + 1)
        v[4] = 0
        return {"rc": synth.uniform_below(3, 2**16 + 2**14, seed=seed + 2), "mb": synth.uniform_below(4, 2**9, seed=seed + 3),
                "mr": mr, "wt": wt, "v": v, "y": y, "s": s, "a": a, "b": b, "in": synth.random_scalars(8, seed=seed + 4)}
    true, stale = one(400), one(500)
    stale["mr"] = true["mr"]  # the bounds are public: they give the circuit its shape
    return true, stale


def append_on_device(comp, t, before=lambda *keys: None):
    """one batched call of each family over the device tensors t (the witnesses are whatever t holds when the kernels run);
    before(keys) runs ahead of each call with the names of the tensors it reads"""
    before("rc")
    comp.range_check_batch(S(5), S(2**16), t["rc"])
    before("mb")
    comp.max_bound_batch(S(2**8 + 3), t["mb"])
    before("mr", "wt")
    comp.max_bound_ragged_batch(t["mr"], t["wt"])
    before("v", "y", "s", "a", "b")
    _, _, nerr = comp.scalar_mix_batch(t["v"], t["y"], t["s"], t["a"], t["b"])
    assert nerr == 1
    before("in")
    first = comp.add_input_batch(t["in"])
    before()
    vars_ = torch.arange(first, first + 8, dtype=torch.int64, device=DEV)
    comp.add_batch(S(3), vars_, S(5), vars_.flip(0), S(7))
    comp.mul_batch(S(11), vars_, vars_.roll(1), S(13))


def append_on_oracle(ora, w):
    from oracle import pyoracle as po
    f = lambda x: po.fr(synth.mont(x))
    nb = C.c_uint64()
    for x in w["rc"]:
        ora.L.range_check(ora.c, f(5), f(2**16), ora.allocate(x))
    for x in w["mb"]:
        ora.L.max_bound(ora.c, f(2**8 + 3), ora.allocate(x), C.byref(nb))
    for bnd, x in zip(w["mr"], w["wt"]):
        ora.L.max_bound(ora.c, po.fr(bnd), ora.allocate(x), C.byref(nb))
    for i in range(len(w["v"])):
        vv, yy, ss = ora.add_input(w["v"][i]), ora.add_input(w["y"][i]), ora.add_input(w["s"][i])
        aa, bb = ora.allocate(w["a"][i]), ora.allocate(w["b"][i])
        ora.L.is_non_zero(ora.c, vv, po.fr(w["v"][i]))
        ora.L.conditionally_select_one(ora.c, yy, ss)
        ora.L.maybe_equal(ora.c, aa, bb)
    vars_ = [ora.add_input(x) for x in w["in"]]
    for a, b in zip(vars_, reversed(vars_)):
        ora.L.composer_add(ora.c, f(3), a, f(5), b, f(7), None)
    for a, b in zip(vars_, vars_[-1:] + vars_[:-1]):
        ora.L.composer_mul(ora.c, f(11), a, b, f(13), None)


def relag(stream):
    """a fresh delay on `stream`, checked to be running: for a call that synchronises the host"""
    ev = lagging(stream)
    assert not ev.query(), LATE
    return ev


def check_composer_against_oracle(engine, comp, ora, lag):
    """every getter of the composer, each behind a fresh delay on the stream `lag`, against the oracle's circuit"""
    n, nv = ora.n, ora.num_vars
    assert (comp.circuit_size(), comp.num_variables()) == (n, nv)
    assert 256 < n < 4096
    padded_n = 1 << (n - 1).bit_length()
    pad = lambda xs: xs + [0] * (padded_n - len(xs))
    exp, full = ora.export(), ora.full_columns()
    wire_cols = [exp["w_l"], exp["w_r"], exp["w_o"], full["w_4"]]
    wire_vals = [exp["var_values"][w.astype(np.int64)] for w in wire_cols]
    wire_ints = [PM.ints_of(v) for v in wire_vals]
    sigma = ora.sigma(padded_n)
    omega = PM.omega_of(padded_n.bit_length() - 1)

    relag(lag)
    got = comp.export()
    for k in exp:
        assert np.array_equal(got[k], exp[k]), k
    relag(lag)
    vals = comp.wire_values()
    for j in range(4):
        assert np.array_equal(host(vals[j]), wire_vals[j]), j
    relag(lag)
    mat = comp.materialize()
    for j, name in enumerate(("w_l_value", "w_r_value", "w_o_value", "w_4_value")):
        assert np.array_equal(host(mat[name]), wire_vals[j]), name
    for name in ("q_4", "q_arith"):
        assert np.array_equal(host(mat[name]), full[name]), name
    assert np.array_equal(host(mat["w_4"]), full["w_4"])
    relag(lag)
    assert np.array_equal(host(comp.permutation(padded_n)), sigma)
    relag(lag)
    assert np.array_equal(host(comp.construct_dense_pi_vec()), full["dense_pi"])
    exp_wp = [NM.ifft(pad(w)) for w in wire_ints]
    for tail in (0, 8):
        relag(lag)
        wp = comp.wire_polynomials(tail=tail)
        assert wp.shape == (4, padded_n + tail, 4)
        for j in range(4):
            assert np.array_equal(host(wp[j, :padded_n]), PM.limbs_of(exp_wp[j])), (tail, j)
        assert not bool(wp[:, padded_n:].any())
    sev = PM.sigma_evaluations(sigma, padded_n, omega)
    exp_sp = [NM.ifft(s) for s in sev]
    relag(lag)
    sp = comp.sigma_polynomials()
    for j in range(4):
        assert np.array_equal(host(sp[j]), PM.limbs_of(exp_sp[j])), j
    columns = dict(exp, q_4=full["q_4"], q_arith=full["q_arith"])
    exp_sel = {name: NM.ifft(pad(PM.ints_of(columns[name]))) if name in columns else [0] * padded_n for name in comp.SELECTORS}
    relag(lag)
    sel = comp.selector_polynomials()
    for name in comp.SELECTORS:
        assert np.array_equal(host(sel[name]), PM.limbs_of(exp_sel[name])), name
    ez, ewrap = PM.grand_product(wire_ints, sigma, padded_n, BETA, GAMMA, omega)
    assert ewrap == 1
    relag(lag)
    pp = comp.prover_polynomials(S(BETA), S(GAMMA))
    for j in range(4):
        assert np.array_equal(host(pp["wires"][j]), PM.limbs_of(exp_wp[j])), j
        assert np.array_equal(host(pp["sigmas"][j]), PM.limbs_of(exp_sp[j])), j
    assert np.array_equal(host(pp["z"]), PM.limbs_of(NM.ifft(ez)))
    for name in engine.QUOTIENT_SELECTORS:
        assert np.array_equal(host(pp["selectors"][name]), PM.limbs_of(exp_sel[name])), name
    assert np.array_equal(host(pp["pi"]), PM.limbs_of(NM.ifft(pad(PM.ints_of(full["dense_pi"])))))
    assert "q_range" not in pp
    relag(lag)
    assert comp.check() == ora.check() == -1
    relag(lag)
    assert comp.copy_constraints_hold()


@functools.lru_cache(maxsize=None)
def mixed_circuit():
    """(the oracle's circuit of the true witnesses, the true witnesses and the stale ones as numpy arrays)"""
    from oracle import pyoracle as po
    true, stale = mixed_circuit_inputs()
    ora, ora_stale = po.Composer(), po.Composer()
    append_on_oracle(ora, true)
    append_on_oracle(ora_stale, stale)
    assert (ora.n, ora.num_vars) == (ora_stale.n, ora_stale.num_vars)
    assert not np.array_equal(ora.export()["var_values"], ora_stale.export()["var_values"])
    return ora, true, stale


def warm_composers(engine, side, t):
    """the appends on throw-away composers of the same engine (its scratch grows), under both streams (torch's allocator)"""
    for s in (torch.cuda.current_stream(), side):
        with torch.cuda.stream(s):
            c0 = pg.StandardComposer(engine, 1 << 13, 1 << 13)
            append_on_device(c0, t)
            c0.sync()
            c0.close()
    torch.cuda.synchronize()


def own_stream(side, made_on):
    """the stream a composer is made on"""
    return torch.cuda.current_stream() if made_on == "default" else side


def other_stream(side, made_on):
    """the stream a composer made on `made_on` is used under: the side stream, or the default one"""
    return side if made_on == "default" else torch.cuda.current_stream()


@pytest.mark.parametrize("made_on", ["default", "side"])
def test_appends_to_a_composer_under_another_stream(engine, side, made_on):
    """made_on = default: the composer is the default stream's, and one batched append of each family runs under the lagging side
    stream, on which the witness tensors get their true values behind the delay (a fresh delay before every call).  made_on =
    side: the mirror image -- the composer is the side stream's, the appends come from the default stream while the side stream
    lags (the witnesses are then the default stream's).  The columns and every Variable must be the oracle's."""
    ora, true, stale = mixed_circuit()
    t_true = {k: dev_np(v) for k, v in true.items()}
    t = {k: dev_np(v) for k, v in stale.items()}
    warm_composers(engine, side, t)

    def true_behind_a_delay(*keys):
        ev = lagging(side)
        for k in keys:
            t[k].copy_(t_true[k])  # (on the current stream)
        assert not ev.query(), LATE
    with torch.cuda.stream(own_stream(side, made_on)):
        comp = pg.StandardComposer(engine, 1 << 13, 1 << 13)
    torch.cuda.synchronize()
    with torch.cuda.stream(other_stream(side, made_on)):
        append_on_device(comp, t, true_behind_a_delay)
        relag(side)
        got = comp.export()
        relag(side)
        assert comp.check() == -1
    torch.cuda.synchronize()
    exp = ora.export()
    assert (comp.circuit_size(), comp.num_variables()) == (ora.n, ora.num_vars)
    for k in exp:
        assert np.array_equal(got[k], exp[k]), k
    comp.close()


@pytest.mark.parametrize("made_on", ["default", "side"])
def test_getters_of_a_composer_under_another_stream(engine, side, made_on):
    """a composer made and filled on one stream (default: the default stream, side: the side stream); every getter is then called
    under the other one, each behind a fresh delay on the side stream -- which is the current stream in the first case and the
    composer's in the second"""
    ora, true, _ = mixed_circuit()
    t = {k: dev_np(v) for k, v in true.items()}
    warm_composers(engine, side, t)
    with torch.cuda.stream(own_stream(side, made_on)):
        comp = pg.StandardComposer(engine, 1 << 13, 1 << 13)
        append_on_device(comp, t)
        comp.sync()
    torch.cuda.synchronize()
    with torch.cuda.stream(other_stream(side, made_on)):
        check_composer_against_oracle(engine, comp, ora, side)
    torch.cuda.synchronize()
    comp.close()


def test_range_gate_batch_under_a_lagging_stream(engine, side):
    """range_gate_batch of a composer made on the default stream, its array of Variables filled in on the lagging side stream
    (stale: other Variables, which hold other values in range), against tests/range_gate_model.py"""
    num_bits, batch = 16, 40
    rng = random.Random(77)
    values = [rng.randrange(2**num_bits) for _ in range(2 * batch)]
    comp = pg.StandardComposer(engine, 1 << 12, 1 << 12)
    first = comp.add_input_batch(dev_np(synth.scalars_from_ints(values)))
    mod = GATE.Circuit(n_rows=comp.circuit_size(), values=[0, 6, 1, 7, GATE.R - 20] + values, zero_var=comp.zero_var)
    assert first == 5 and comp.num_variables() == len(mod.values)
    n0, nv0 = comp.circuit_size(), comp.num_variables()
    true = list(range(first, first + batch))
    stale = list(range(first + batch, first + 2 * batch))
    wv = torch.tensor(stale, dtype=torch.int64, device=DEV)
    t_true = torch.tensor(true, dtype=torch.int64, device=DEV)
    c0 = pg.StandardComposer(engine, 1 << 12, 1 << 12)  # warm-up on another composer, under both streams
    c0.add_input_batch(dev_np(synth.scalars_from_ints(values)))
    c0.range_gate_batch(wv, num_bits)
    with torch.cuda.stream(side):
        c0.range_gate_batch(wv, num_bits)
    c0.sync()
    c0.close()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ev = lagging(side)
        wv.copy_(t_true)
        assert not ev.query(), LATE
        comp.range_gate_batch(wv, num_bits)  # (it checks its Variables first: a host synchronisation)
        relag(side)
        got = comp.export(n0, nv0)
        relag(side)
        q_range = comp.materialize()["q_range"]
        relag(side)
        assert comp.check() == -1
        relag(side)
        assert comp.copy_constraints_hold()
    torch.cuda.synchronize()
    for w in true:
        mod.range_gate(w, num_bits)
    rows = mod.rows[n0:]
    assert comp.circuit_size() == len(mod.rows) and comp.num_variables() == len(mod.values)
    for j, k in enumerate(("w_l", "w_r", "w_o")):
        assert np.array_equal(got[k], np.array([r[j] for r in rows], dtype=np.uint64)), k
    assert np.array_equal(got["var_values"].reshape(-1, 4), synth.scalars_from_ints(mod.values[nv0:]))
    one = np.array(synth.mont(1), dtype=np.uint64)
    exp_q = np.zeros((len(mod.rows), 4), dtype=np.uint64)
    exp_q[np.array(mod.q_range, dtype=bool)] = one
    assert np.array_equal(host(q_range), exp_q)
    comp.close()


# ---- D. end to end ----------------------------------------------------------------------------------------------------------
FIXED_BLINDERS = [0x5EED_0B00 + 7 * i for i in range(11)]


def small_circuit(engine, with_range_gate):
    """a satisfied circuit of a few hundred rows with one public input"""
    comp = pg.StandardComposer(engine, 1 << 12, 1 << 12)
    comp.range_check_batch(S(5), S(2**16), dev_np(synth.uniform_below(3, 2**16, seed=600)))
    comp.max_bound_batch(S(2**8 + 3), dev_np(synth.uniform_below(4, 2**8, seed=601)))
    x = comp.add_input(S(9))
    comp.constrain_to_constant(x, S(20), S(11))  # 9 - 20 + PI = 0
    if with_range_gate:
        first = comp.add_input_batch(dev_np(synth.scalars_from_ints([0, 2**10 - 1, 513, 77])))
        comp.range_gate_batch(torch.arange(first, first + 4, dtype=torch.int64, device=DEV), 10)
    comp.sync()
    return comp


@pytest.fixture(scope="module")
def keys(engine):
    ck = pg.CommitKey.setup(engine, (1 << 11) - 1, S(TAU))
    ok = pg.OpeningKey.setup(engine, S(TAU))
    torch.cuda.synchronize()
    yield ck, ok
    ok.close()


@pytest.fixture(scope="module")
def proven(engine, side, keys):
    """[(proof from the default stream, proof under the lagging side stream, verifier key, public inputs)] for the three kinds of
    proof; the composers are made on the default stream"""
    ck, _ = keys
    out = {}
    for kind, with_gate, blinding in (("unblinded", False, None), ("fixed_blinders", False, FIXED_BLINDERS),
                                      ("range_gate", True, FIXED_BLINDERS)):
        comp = small_circuit(engine, with_gate)
        assert comp.check() == -1 and comp.circuit_size() < 1 << 10
        pre = comp.preprocessed_commitments(ck)
        plain = comp.prove(ck, b"plonk", pre, blinding=blinding)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            comp.prove(ck, b"plonk", pre, blinding=blinding)  # (warm: this stream's blocks in torch's allocator)
            torch.cuda.synchronize()
            relag(side)
            lagged = comp.prove(ck, b"plonk", pre, blinding=blinding)
        torch.cuda.synchronize()
        dense = host(comp.construct_dense_pi_vec())
        pi = {i: synth.to_int(row) for i, row in enumerate(dense.tolist()) if any(row)}
        padded_n = 1 << (comp.circuit_size() - 1).bit_length()
        out[kind] = (plain, lagged, pg.VerifierKey(padded_n, pre), pi, pre, padded_n)
        comp.close()
    return out


@pytest.mark.parametrize("kind", ["unblinded", "fixed_blinders", "range_gate"])
def test_prove_under_a_lagging_stream_gives_the_same_bytes(proven, kind):
    plain, lagged, vk, pi, pre, padded_n = proven[kind]
    assert pi == {[i for i in pi][0]: 11}
    assert lagged.to_bytes() == plain.to_bytes()
    if kind != "range_gate":  # (the trapdoor verifier of tests/plonk_verify_model.py knows no range widget)
        assert VM.verify(plain, pre, pi, padded_n, TAU)


def flipped(proof, at):
    raw = bytearray(proof.to_bytes())
    raw[at] ^= 1
    return bytes(raw)


def test_plonk_sides_and_the_pairing_check_on_proofs_that_arrive_on_the_lagging_stream(engine, side, keys, proven):
    """verify_encoded of a device tensor of proofs -- pg_plonk_sides, pg_msm_segmented and pg_pairing_check enqueued one behind the
    other -- whose bytes are written behind the delay; the verdicts are the trapdoor verifier's (tests/plonk_verify_model.py)"""
    _, ok = keys
    kinds = ["unblinded", "fixed_blinders"]
    vks, pis = [proven[k][2] for k in kinds], [proven[k][3] for k in kinds]
    good = [proven[k][0].to_bytes() for k in kinds]
    bad = [flipped(proven[k][0], 11 * 48 + 5 * 32 + 3) for k in kinds]
    for k, g, b in zip(kinds, good, bad):
        _, _, _, pi, pre, padded_n = proven[k]
        assert VM.verify(pg.Proof.from_bytes(g), pre, pi, padded_n, TAU) and not VM.verify(pg.Proof.from_bytes(b), pre, pi, padded_n, TAU)
    on_device = lambda parts: torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).view(2, 1040).to(DEV)
    buf = torch.empty((2, 1040), dtype=torch.uint8, device=DEV)
    call = lambda: pg.verify_encoded(buf, vks, ok, pis)
    assert behind(side, [(buf, on_device(bad), on_device(good))], call, enqueues=False) == [True, True]
    assert behind(side, [(buf, on_device(good), on_device([good[0], bad[1]]))], call, enqueues=False, warm=False) == [True, False]


def test_the_verifiers_under_a_lagging_stream(engine, side, keys, proven):
    """verify, verify_each, verify_batch and verify_encoded accept the three proofs and reject one flipped byte of an evaluation,
    each called behind a fresh delay"""
    _, ok = keys
    kinds = list(proven)
    proofs = [proven[k][0] for k in kinds]
    vks = [proven[k][2] for k in kinds]
    pis = [proven[k][3] for k in kinds]
    at = 11 * 48 + 5 * 32 + 3  # a byte of b_next_eval
    bad = pg.Proof.from_bytes(flipped(proofs[1], at))
    mixed = [proofs[0], bad, proofs[2]]
    for warm in (True, False):  # once without a delay (scratch, allocator), then behind delays
        with torch.cuda.stream(side):
            lag = (lambda: None) if warm else (lambda: relag(side))
            lag()
            assert all(pg.verify(p, vk, ok, pi) for p, vk, pi in zip(proofs, vks, pis))
            lag()
            assert not pg.verify(bad, vks[1], ok, pis[1])
            lag()
            assert pg.verify_each(proofs, vks, ok, pis) == [True, True, True]
            lag()
            assert pg.verify_each(mixed, vks, ok, pis) == [True, False, True]
            lag()
            assert pg.verify_batch(proofs, vks, ok, pis) is True
            lag()
            assert pg.verify_batch(mixed, vks, ok, pis) is False
            # (verify_encoded refuses a key with range_gate items: the first two)
            lag()
            assert pg.verify_encoded(b"".join(p.to_bytes() for p in proofs[:2]), vks[:2], ok, pis[:2]) == [True, True]
            lag()
            assert pg.verify_encoded(b"".join(p.to_bytes() for p in mixed[:2]), vks[:2], ok, pis[:2]) == [True, False]
        torch.cuda.synchronize()
