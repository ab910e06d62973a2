"""GPU: csrc/fr.hpp's device forms -- the gfx950 carry chains and product scanning of fr_add / fr_sub / fr_mul, the
division-step inversion with its wave-wide early exit -- one operation at a time against the big-integer model
(tests/fr_model.py), limb for limb, on the edge corpus and on uniform pairs, in three launch shapes: full occupancy, one
wave per workgroup (a wave alone on its SIMD, issuing back to back) and workgroups of 96 lanes (a partial wave in each).
The harness is tests/cpp/fr_device_ops.hip; the product ABI's own conversions are checked without it."""
import ctypes as C
import random

import numpy as np
import pytest

import fr_model as fm

pytestmark = pytest.mark.gpu

Q = fm.Q
N_UNIFORM = 1 << 20        # uniform pairs in the full-occupancy run (the other shapes take N_UNIFORM_SHAPE)
N_UNIFORM_SHAPE = 1 << 14
CHAIN_LANES, CHAIN_STEPS = 16384, 3000
SHAPES = {"full": (256, None), "wave_alone": (64, 256), "partial_wave": (96, None)}  # block, grid cap (None: cover n)


@pytest.fixture(scope="module")
def ops():
    import sys
    import os
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp"))
    import fr_device_build
    lib = C.CDLL(fr_device_build.build())
    P, U64, I = C.c_void_p, C.c_uint64, C.c_int
    sigs = {"fr_dev_unary": [I, P, P, U64, I, I], "fr_dev_binary": [I, P, P, P, U64, I, I], "fr_dev_pow_of_2": [P, P, U64, I, I],
            "fr_dev_bits": [P, P, P, U64, I, I], "fr_dev_chain": [P, P, P, U64, C.c_uint32, I, I],
            "fr_dev_masked_invert": [P, P, P, U64, I, I], "fr_host_chain": [P, P, P, U64, C.c_uint32, I]}
    for name, args in sigs.items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, I
    assert torch.cuda.is_available()
    return lib


def dev(values):
    import torch
    raw = b"".join(int(x).to_bytes(32, "little") for x in values)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.int64).reshape(-1, 4).copy()).to("cuda:0")


def ints(t):
    import torch
    torch.cuda.synchronize()
    raw = t.cpu().numpy().astype(np.int64).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


def shape(name, n):
    block, cap = SHAPES[name]
    grid = max(1, -(-n // block))
    return block, min(grid, cap) if cap else grid


def run_unary(lib, op, values, shp):
    import torch
    a = dev(values)
    out = torch.full_like(a, -1)
    assert lib.fr_dev_unary(op, a.data_ptr(), out.data_ptr(), len(values), *shape(shp, len(values))) == 0
    return ints(out)


def run_binary(lib, op, pairs, shp):
    import torch
    a, b = dev([p[0] for p in pairs]), dev([p[1] for p in pairs])
    out = torch.full_like(a, -1)
    assert lib.fr_dev_binary(op, a.data_ptr(), b.data_ptr(), out.data_ptr(), len(pairs), *shape(shp, len(pairs))) == 0
    return ints(out)


def uniform_pairs(n, seed):
    rng = random.Random(seed)
    return [(rng.randrange(Q), rng.randrange(Q)) for _ in range(n)]


def check(name, got, want, inputs):
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{name}: {len(bad)} of {len(want)} differ, first input {[hex(x) for x in inputs[bad[0]]]}: " \
                    f"device {hex(got[bad[0]])}, model {hex(want[bad[0]])}"
    assert max(got) < Q


@pytest.mark.parametrize("shp", list(SHAPES))
def test_elementwise_ops_on_the_corpus_and_uniform_pairs(ops, shp):
    pairs = fm.corpus_pairs() + uniform_pairs(N_UNIFORM if shp == "full" else N_UNIFORM_SHAPE, seed=11)
    compared = 0
    for op, f in ((0, fm.add), (1, fm.sub), (2, fm.mul)):
        check(f.__name__, run_binary(ops, op, pairs, shp), [f(a, b) for a, b in pairs], pairs)
        compared += len(pairs)
    values = [p[0] for p in pairs] + [p[1] for p in pairs[:4096]]
    for op, f in ((0, fm.neg), (1, fm.square), (2, fm.to_mont), (3, fm.from_mont)):
        check(f.__name__, run_unary(ops, op, values, shp), [f(a) for a in values], [(a,) for a in values])
        compared += len(values)
    inv = list(fm.corpus_values()) + [a for a, _ in uniform_pairs(4096, seed=12)]
    want = [fm.invert(a) for a in inv]
    check("invert_or_zero", run_unary(ops, 4, inv, shp), want, [(a,) for a in inv])
    check("invert_fermat", run_unary(ops, 5, inv, shp), want, [(a,) for a in inv])
    compared += 2 * len(inv)
    print(f"{shp}: {compared} device results compared, {len(fm.corpus_pairs())} corpus pairs, "
          f"{len(fm.corpus_values())} corpus values; classes {({k: len(v) for k, v in fm.corpus().items()})}")


@pytest.mark.parametrize("shp", ["full", "wave_alone"])
def test_dependent_chains_match_the_host_chain_and_python_ints(ops, shp):
    import torch
    rng = random.Random(21)
    vals = list(fm.corpus_values())
    xs = [rng.choice(vals) if i % 4 == 0 else rng.randrange(Q) for i in range(CHAIN_LANES)]
    ys = [rng.choice(vals) if i % 4 == 1 else rng.randrange(Q) for i in range(CHAIN_LANES)]
    x, y = dev(xs), dev(ys)
    out = torch.full_like(x, -1)
    assert ops.fr_dev_chain(x.data_ptr(), y.data_ptr(), out.data_ptr(), CHAIN_LANES, CHAIN_STEPS, *shape(shp, CHAIN_LANES)) == 0
    got = ints(out)
    hx, hy = x.cpu().contiguous(), y.cpu().contiguous()
    host = torch.full_like(hx, -1)
    assert ops.fr_host_chain(hx.data_ptr(), hy.data_ptr(), host.data_ptr(), CHAIN_LANES, CHAIN_STEPS, 16) == 0
    want = [int.from_bytes(host.numpy().tobytes()[32 * i:32 * i + 32], "little") for i in range(CHAIN_LANES)]
    check("chain vs host", got, want, list(zip(xs, ys)))
    for i in (0, 1, 63, CHAIN_LANES - 1):  # a reference that does not depend on fr.hpp
        assert got[i] == fm.chain(xs[i], ys[i], CHAIN_STEPS), i
    print(f"{shp}: {CHAIN_LANES} lanes x {CHAIN_STEPS} steps ({3 * CHAIN_LANES * CHAIN_STEPS} dependent operations)")


def slow_input():
    return max(fm.corpus_values(), key=fm.invert_steps)


@pytest.mark.parametrize("block", [64, 256])
def test_inversion_waits_for_its_slowest_lane(ops, block):
    """one slow input (the corpus' most division steps) at lane 0, 31, 32 or 63 of a wave whose other lanes hold 0 (done
    after one batch) or 1"""
    slow = slow_input()
    assert fm.invert_batches(slow) >= 18
    vals = []
    for filler in (0, 1):
        for lane in (0, 31, 32, 63):
            w = [filler] * 64
            w[lane] = slow
            vals += w
    got = run_unary(ops, 4, vals, "full" if block == 256 else "wave_alone")
    check("invert layouts", got, [fm.invert(a) for a in vals], [(a,) for a in vals])


def test_masked_inversion_in_a_divergent_branch(ops):
    import torch
    slow = slow_input()
    rng = random.Random(31)
    vals, act = [], []
    for lane in (0, 31, 32, 63):
        for slow_active in (True, False):
            # the zeros are active (done after one batch), the other values inactive: the slow lane alone decides
            w = [0 if rng.random() < 0.5 else rng.randrange(Q) for _ in range(64)]
            a = [x == 0 for x in w]
            w[lane], a[lane] = slow, slow_active
            vals += w
            act += a
    n = len(vals) - 31  # and a partial last wave
    vals, act = vals[:n], act[:n]
    a = dev(vals)
    m = torch.tensor(act, dtype=torch.uint8, device="cuda:0")
    out = torch.full_like(a, -1)
    for block in (64, 256):
        assert ops.fr_dev_masked_invert(a.data_ptr(), m.data_ptr(), out.data_ptr(), n, block, -(-n // block)) == 0
        check("masked invert", ints(out), [fm.invert(v) if on else v for v, on in zip(vals, act)], [(v,) for v in vals])


def test_inversion_in_a_partial_last_wave(ops):
    slow = slow_input()
    vals = [fm.mont(i) for i in range(64 * 3)] + [0] * 12 + [slow]
    for shp in SHAPES:
        check("invert partial", run_unary(ops, 4, vals, shp), [fm.invert(a) for a in vals], [(a,) for a in vals])


def test_pow_of_2_and_bit_counts(ops):
    import torch
    by = torch.arange(0, 301, dtype=torch.int64, device="cuda:0")
    out = torch.full((301, 4), -1, dtype=torch.int64, device="cuda:0")
    assert ops.fr_dev_pow_of_2(by.data_ptr(), out.data_ptr(), 301, 64, 5) == 0
    check("pow_of_2", ints(out), [fm.pow_of_2(k) for k in range(301)], [(k,) for k in range(301)])
    canon = sorted({(1 << k) % Q for k in range(256)} | {((1 << k) - 1) % Q for k in range(257)} | {Q - 1, Q - 2})
    vals = [fm.mont(c) for c in canon] + canon  # the values themselves, and as Montgomery residues
    a = dev(vals)
    cnt = torch.full((len(vals),), -1, dtype=torch.int64, device="cuda:0")
    close = torch.full_like(cnt, -1)
    assert ops.fr_dev_bits(a.data_ptr(), cnt.data_ptr(), close.data_ptr(), len(vals), 96, -(-len(vals) // 96)) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [fm.bits_count(v) for v in vals]
    assert close.cpu().tolist() == [fm.num_bits_closest_power_of_two(v) for v in vals]


def test_product_abi_canonical_conversions_at_the_modulus():
    """pg_scalars_from_canonical_batch / to_canonical (the product's own kernels, no harness): the comparison with q is
    decided at each limb in turn"""
    import plonk_gadgets_amd as pg
    raws = [Q - 1, Q, Q + 1, (1 << 256) - 1, 0, 1]
    for i in range(4):
        raws += [Q + (1 << (64 * i)), Q - (1 << (64 * i))]
    raws = [r for r in raws if r < 1 << 256]
    eng = pg.Engine(0)
    try:
        out, bad, count = eng.scalars_from_canonical(dev(raws))
        assert bad.cpu().tolist() == [int(r >= Q) for r in raws]
        assert count == sum(r >= Q for r in raws)
        assert ints(out) == [fm.to_mont(r) if r < Q else 0 for r in raws]
        vals = list(fm.corpus_values())
        canon = eng.scalars_to_canonical(dev(vals))
        assert ints(canon) == [fm.from_mont(v) for v in vals]
        back, bad, count = eng.scalars_from_canonical(canon)
        assert count == 0 and int(bad.sum()) == 0 and ints(back) == vals
    finally:
        eng.close()
