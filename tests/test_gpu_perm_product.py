"""GPU: pg_sigma_evaluations and pg_permutation_product (csrc/permutation_product.hpp) against the Python-int model of
tests/perm_product_model.py, limb for limb, on small circuits of every append kind the f-row tests build; the copy constraints of
those circuits hold (wrap == 1, StandardComposer.copy_constraints_hold), and stop holding when a wire value or sigma is corrupted;
the error cases; synthetic cycles over 2^24 rows (the first size at which launch 1 reuses its denominator slabs and a lane of
launch 2 carries more than one tile), z checked by the recurrence on the host; and the 270 M-row composer of bench.py padded to
2^29, checked the same way."""
import os
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perm_product_model as M  # noqa: E402

DEV = "cuda:0"
S = pg.BlsScalar.from_int
BETA, GAMMA = 0x5EED_0001 ** 9 % M.Q, 0x5EED_0002 ** 11 % M.Q


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint64)


def build(engine, kind):
    """a small circuit of one append kind (the kinds of tests/test_gpu_frows_exhaustive.py)"""
    import bench
    comp = pg.StandardComposer(engine, 1 << 17, 1 << 17)
    if kind == "ladders":            # allocate + range_check, and max_bound, as batched calls
        comp.range_check_batch(S(0), S(2**254), dev(synth.random_scalars(9, seed=11)))
        comp.max_bound_batch(S(2**100 + 7), dev(synth.random_scalars(5, seed=12)))
    elif kind == "allocated":        # witnesses allocated first, then range_check over them
        wit = synth.random_scalars(7, seed=13)
        first = comp.add_input_batch(dev(wit))
        comp.range_check_allocated_batch(S(0), S(2**200), torch.arange(first, first + 7, device=DEV), dev(wit))
    elif kind == "per_item_bounds":
        mr, wt = bench.c4_inputs(24, seed=14)
        comp.max_bound_ragged_batch(dev(mr), dev(wt))
    elif kind == "mix_with_failing_items":
        v, y, s, a, b = bench.mix_inputs(700, seed=15)
        v[::7] = 0                   # is_non_zero fails on these items
        _, _, nerr = comp.scalar_mix_batch(*[dev(x) for x in (v, y, s, a, b)])
        assert nerr > 0
    elif kind == "gate_batches":     # the small gadgets and the gate batches on Variables from everywhere
        rng = np.random.default_rng(16)
        first = comp.add_input_batch(dev(synth.random_scalars(600, seed=16)))
        nv = lambda: comp.num_variables()
        pick = lambda: torch.from_numpy(rng.integers(0, nv(), size=600).astype(np.int64)).to(DEV)
        comp.conditionally_select_zero_batch(pick(), pick())
        comp.conditionally_select_one_batch(pick(), pick())
        comp.maybe_equal_batch(pick(), pick())
        comp.is_non_zero_batch(torch.arange(first, first + 600, device=DEV))
        comp.add_batch(S(3), pick(), S(5), pick(), S(7))
        comp.mul_batch(S(11), pick(), pick(), S(13))
        comp.poly_gate_batch(pick(), pick(), pick(), S(1), S(2), S(3), S(4), S(5))
        comp.constrain_to_constant_batch(pick(), S(7))
        comp.boolean_gate_batch(pick())
    elif kind == "single_calls":     # the reference tests' loop, call by call through the command queue
        comp.queue(True)
        for i, w in enumerate((5, 70_000, 249_999, 250_001, 3)):
            r = pg.range_check(comp, S(50_000), S(250_000), pg.AllocatedScalar.allocate(comp, S(w)))
            comp.constrain_to_constant(r, S(int(50_000 <= w <= 250_000)), None)
        a = pg.AllocatedScalar.allocate(comp, S(9))
        b = pg.AllocatedScalar.allocate(comp, S(9))
        pg.maybe_equal(comp, a, b)
        pg.is_non_zero(comp, a.var, S(9))
        comp.sync()
    else:
        raise AssertionError(kind)
    # (gates on random Variables are not satisfied -- their copy constraints hold all the same)
    assert comp.check() == -1 or kind == "gate_batches"
    return comp


KINDS = ["ladders", "allocated", "per_item_bounds", "mix_with_failing_items", "gate_batches", "single_calls"]


@pytest.mark.parametrize("kind", KINDS)
def test_small_circuits_equal_the_model(engine, kind):
    comp = build(engine, kind)
    n = comp.circuit_size()
    # one domain well above the circuit, the others the next power of two; n_values = circuit_size
    padded_n = 1 << ((n - 1).bit_length() + (2 if kind == "ladders" else 0))
    m = padded_n.bit_length() - 1
    omega = M.omega_of(m)
    sigma = comp.permutation(padded_n)
    vals = comp.wire_values()
    hs = host(sigma)
    wires = [M.ints_of(host(v)) for v in vals]
    # sigma evaluations, every entry
    ev = engine.sigma_evaluations(sigma)
    exp = M.sigma_evaluations(hs, padded_n, omega)
    assert np.array_equal(host(ev).reshape(4 * padded_n, 4), M.limbs_of([x for j in range(4) for x in exp[j]]))
    # z and wrap, every entry
    z, wrap = engine.permutation_product(vals, sigma, S(BETA), S(GAMMA))
    ez, ewrap = M.grand_product(wires, hs, padded_n, BETA, GAMMA, omega)
    assert ewrap == 1 and wrap.to_int() == 1
    assert np.array_equal(host(z), M.limbs_of(ez))
    assert comp.copy_constraints_hold()
    assert comp.copy_constraints_hold(beta=S(7), gamma=S(11), padded_n=2 * padded_n)
    comp.close()


def test_corruptions_break_the_copy_constraints(engine):
    comp = build(engine, "ladders")
    n = comp.circuit_size()
    padded_n = 1 << (n - 1).bit_length()
    sigma = comp.permutation(padded_n)
    vals = comp.wire_values()
    assert engine.permutation_product(vals, sigma, S(BETA), S(GAMMA))[1].to_int() == 1
    hs = host(sigma)
    row = next(i for i in range(3, n) if hs[0, i] != i)  # a position on a cycle of more than one
    # one wire value changed in one row
    bad = [v.clone() for v in vals]
    bad[0][row, 0] += 1
    assert engine.permutation_product(bad, sigma, S(BETA), S(GAMMA))[1].to_int() != 1
    # two sigma entries swapped between positions of different Variables
    w_l = host(comp.device_columns().w_l)
    j = next(j for j in range(3, n) if w_l[j] != w_l[row] and hs[0, j] != j)
    sw = sigma.clone()
    sw[0, row], sw[0, j] = sigma[0, j], sigma[0, row]
    assert engine.permutation_product(vals, sw, S(BETA), S(GAMMA))[1].to_int() != 1
    # the same corruptions through copy_constraints_hold
    assert comp.copy_constraints_hold()
    comp.wire_values = lambda: bad
    assert not comp.copy_constraints_hold()
    del comp.wire_values
    comp.permutation = lambda padded_n=None: sw
    assert not comp.copy_constraints_hold()
    del comp.permutation
    assert comp.copy_constraints_hold()
    comp.close()


def test_error_cases(engine):
    comp = build(engine, "ladders")
    n = comp.circuit_size()
    padded_n = 1 << (n - 1).bit_length()
    sigma = comp.permutation(padded_n)
    vals = comp.wire_values()
    assert bool((vals[3] == 0).all(dim=1).any())  # the fourth wire holds zero_var: a zero value
    with pytest.raises(pg.NonExistingInverse):
        engine.permutation_product(vals, sigma, S(0), S(0))
    # a padded_n that is not a power of two
    odd = sigma[:, : padded_n - 5].contiguous()
    for call in (lambda: engine.sigma_evaluations(odd, omega=S(5)),
                 lambda: engine.permutation_product([v[: padded_n - 5] for v in vals], odd, S(BETA), S(GAMMA), omega=S(5))):
        with pytest.raises(pg.PgError) as ex:
            call()
        assert ex.value.status == 2 and "power of two" in str(ex.value)
    # n_values above padded_n
    with pytest.raises(pg.PgError) as ex:
        engine.permutation_product(vals, sigma[:, : padded_n // 4].contiguous(), S(BETA), S(GAMMA))
    assert ex.value.status == 2
    # a sigma entry >= 4 * padded_n: reported, nothing read out of bounds
    for big in (4 * padded_n, 4 * padded_n + 3, 2**63 - 1):
        bad = sigma.clone()
        bad[1, 17] = big
        for call in (lambda: engine.sigma_evaluations(bad), lambda: engine.permutation_product(vals, bad, S(BETA), S(GAMMA))):
            with pytest.raises(pg.PgError) as ex:
                call()
            assert ex.value.status == 2 and "sigma" in str(ex.value)
    # and the engine goes on
    assert engine.permutation_product(vals, sigma, S(BETA), S(GAMMA))[1].to_int() == 1
    comp.close()


def synthetic_cycles(padded_n, n_values, seed, device):
    """wire values and a sigma whose cycles pair DISTANT rows, built with torch: for r < padded_n / 2 and its mirror row
    q = padded_n - 1 - r,
      r % 3 == 0: (j, r) <-> (j, q) in every wire j, with equal values;
      r % 3 == 1: (j, r) -> (j + 1 mod 4, q) and (j, q) -> (j + 1 mod 4, r): two cycles of four, the value a of (0, r) on the one
                  through (0, r) and the value b of (0, q) on the other;
      r % 3 == 2: fixed points with unrelated values.
    The rows >= n_values read as zero, so their mirror rows are zero too.  -> (four int64[n_values, 4], sigma int64[4, padded_n])"""
    N = padded_n
    gen = torch.Generator(device=device).manual_seed(seed)
    vals = torch.randint(-(2**63), 2**63 - 1, (4, N, 4), dtype=torch.int64, device=device, generator=gen)
    vals[..., 3] = (vals[..., 3] & (2**63 - 1)) % synth.Q_TOP
    sigma = torch.arange(4 * N, dtype=torch.int64, device=device).view(4, N).clone()
    r = torch.arange(N // 2, dtype=torch.int64, device=device)
    r0, r1 = r[r % 3 == 0], r[r % 3 == 1]
    q0, q1 = N - 1 - r0, N - 1 - r1
    a, b = vals[0, r1].clone(), vals[0, q1].clone()
    for j in range(4):
        sigma[j, r0], sigma[j, q0] = j * N + q0, j * N + r0
        vals[j, q0] = vals[j, r0]
        up = (j + 1) % 4 * N
        sigma[j, r1], sigma[j, q1] = up + q1, up + r1
        vals[j, r1], vals[j, q1] = (a, b) if j % 2 == 0 else (b, a)
    vals[:, : N - n_values] = 0
    return [vals[j, :n_values].contiguous() for j in range(4)], sigma


def test_synthetic_cycles_equal_the_model_at_256_rows(engine):
    """the construction of the 2^24-row test below, small enough for the model: its copy constraints hold, z moves, and a
    bumped value breaks them -- in the model and on the device alike"""
    N, n_values = 256, 256 - 4 * 3
    wires, sigma = synthetic_cycles(N, n_values, seed=256, device=DEV)
    hs, omega = host(sigma), M.omega_of(8)
    ints = [M.ints_of(host(w)) for w in wires]
    ez, ewrap = M.grand_product(ints, hs, N, BETA, GAMMA, omega)
    assert ewrap == 1 and ez[0] == 1 and len(set(ez)) > N // 4
    ratios_not_one = sum(ez[i + 1] != ez[i] for i in range(N - 1))
    assert ratios_not_one >= N // 2
    z, wrap = engine.permutation_product(wires, sigma, S(BETA), S(GAMMA))
    assert wrap.to_int() == 1 and np.array_equal(host(z), M.limbs_of(ez))
    ints[2][100] = (ints[2][100] + 1) % M.Q
    bz, bwrap = M.grand_product(ints, hs, N, BETA, GAMMA, omega)
    assert bwrap != 1
    wires[2] = dev(M.limbs_of(ints[2]))
    z, wrap = engine.permutation_product(wires, sigma, S(BETA), S(GAMMA))
    assert wrap.to_int() == bwrap and np.array_equal(host(z), M.limbs_of(bz))


def product_launches(padded_n, cus):
    """pg_permutation_product's launch arithmetic (capi.hip, permutation_product.hpp): (tiles of 16384 rows, workgroups of
    launch 1 -- two per CU, each reusing its slab of denominators for tiles grid apart --, tiles per lane of launch 2)"""
    tile, threads = 16384, 256  # kPpTile, kThreads
    tiles = (padded_n + tile - 1) // tile
    return tiles, min(tiles, 2 * cus), (tiles + threads - 1) // threads


def test_strided_tiles_and_many_tiles_per_carry_lane(engine):
    """padded_n = the first power of two with more tiles than launch 1 has workgroups (2 per CU) and than launch 2 has lanes
    (256): 2^24 on 256 CUs.  wrap == 1 and z[0] == 1; a bumped value in tile 0 and one in a tile past launch 1's grid each
    make wrap != 1; z[i+1] den_i == z[i] num_i in Python integers at the last row of every tile, at every 64-row lane boundary of
    the first and last tiles, the tiles on either side of launch 1's grid and two random ones, around n_values and at 1000
    random rows; the sigma evaluations at the same rows."""
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (8 << 30):
        pytest.skip("less than 8 GiB of HBM free")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m = next(m for m in range(14, 33) if product_launches(1 << m, cus)[0] > max(2 * cus, 256))
    padded_n = 1 << m
    tiles, grid, per = product_launches(padded_n, cus)
    print("permutation product: %d CUs, padded_n = 2^%d, %d tiles, launch 1 grid %d, %d tiles per carry lane"
          % (cus, m, tiles, grid, per))
    assert tiles > 2 * cus and tiles > 256 and grid == 2 * cus < tiles and per > 1
    assert product_launches(padded_n // 2, cus)[0] <= max(2 * cus, 256)
    tile = 16384
    n_values = padded_n - 4 * 3089  # (not tile-aligned)
    wires, sigma = synthetic_cycles(padded_n, n_values, seed=m, device=DEV)
    omega = M.omega_of(m)
    z, wrap = engine.permutation_product(wires, sigma, S(BETA), S(GAMMA))
    assert wrap.to_int() == 1
    assert M.ints_of(host(z[:1])) == [1]
    rng = np.random.default_rng(m)
    special = [0, tiles - 1, 2 * cus - 1, 2 * cus] + [int(t) for t in rng.integers(1, tiles - 1, size=2)]
    rows = [np.arange(1, tiles + 1) * tile - 1]                                       # the last row of every tile
    rows += [t * tile + np.arange(1, 257) * 64 - 1 for t in special]                  # the last row of every lane's run
    rows += [t * tile + np.arange(0, 256) * 64 for t in special]                      # ... and the first
    rows.append(n_values + np.arange(-3, 3))
    rows.append(rng.integers(0, padded_n, size=1000))
    idx = np.unique(np.concatenate(rows))
    idx = idx[idx < padded_n - 1]
    ti = torch.from_numpy(idx.astype(np.int64)).to(DEV)
    zi = M.ints_of(host(z.index_select(0, ti)))
    zn = M.ints_of(host(z.index_select(0, ti + 1)))
    si = host(sigma.index_select(1, ti))
    live = torch.clamp(ti, max=n_values - 1)
    wv = [M.ints_of(host(w.index_select(0, live))) for w in wires]
    moved = 0
    for r, i in enumerate(idx.tolist()):
        w = [[wv[j][r] if i < n_values else 0] for j in range(4)]
        sev = [M.K[int(x) // padded_n] * pow(omega, int(x) % padded_n, M.Q) % M.Q for x in si[:, r]]
        num, den = M.factors(w, sev, 0, BETA, GAMMA, pow(omega, i, M.Q))
        assert zn[r] * den % M.Q == zi[r] * num % M.Q, i
        moved += num != den
    assert moved >= len(idx) // 2  # (z actually moves: most sampled rows have a ratio other than 1)
    del z
    # one value bumped: in tile 0 (a zeroed mirror row on a swap), and in a tile launch 1 reaches on its second round
    far = next(i for i in range((2 * cus + 1) * tile + 5, n_values) if (padded_n - 1 - i) % 3 == 0)
    assert far // tile >= 2 * cus
    for j, row in ((0, 3), (2, far)):
        bad = list(wires)
        bad[j] = wires[j].clone()
        bad[j][row, 0] += 1
        assert engine.permutation_product(bad, sigma, S(BETA), S(GAMMA))[1].to_int() != 1, (j, row)
        del bad
    del wires
    gc.collect()
    torch.cuda.empty_cache()
    # the sigma evaluations at the same rows, every wire
    ev = engine.sigma_evaluations(sigma)
    for j in range(4):
        got = host(ev[j].index_select(0, ti))
        exp = [M.K[int(x) // padded_n] * pow(omega, int(x) % padded_n, M.Q) % M.Q for x in si[j]]
        assert np.array_equal(got, M.limbs_of(exp)), j
    del ev, sigma
    gc.collect()
    torch.cuda.empty_cache()


def test_full_size_next_rows_composer(engine):
    """bench.py's next_rows composer: 2^18 x (allocate + range_check(0, 2^254)) = 270 270 467 rows, padded to 2^29: wrap == 1;
    z[i+1] den_i == z[i] num_i on the host for every row of the first, the last and two random tiles and across every tile
    boundary; the sigma evaluations at sampled positions and on stretches of wire 0's identity padding"""
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < (170 << 30):
        pytest.skip("not enough free HBM for the 270 M-row composer, its wire values, sigma and z (and then its sigma evaluations)")
    batch = 1 << 18
    comp = pg.StandardComposer(engine, 3 + batch * 1031 + 8, 5 + batch * 1034 + 8)
    comp.range_check_batch(S(0), S(2**254), dev(synth.random_scalars(batch, seed=synth.SEED + 2)))
    n = comp.circuit_size()
    padded_n = 1 << 29
    assert n == 270_270_467 and (1 << (n - 1).bit_length()) == padded_n
    omega = M.omega_of(29)
    sigma = comp.permutation(padded_n)
    vals = comp.wire_values()
    z, wrap = engine.permutation_product(vals, sigma, S(BETA), S(GAMMA))
    assert wrap.to_int() == 1
    tile = 16384
    tiles = padded_n // tile
    rng = np.random.default_rng(29)
    rows = [np.arange(0, tile), np.arange(padded_n - tile, padded_n - 1)]
    rows += [np.arange(t * tile, (t + 1) * tile) for t in rng.integers(1, tiles - 1, size=2)]
    rows.append(np.arange(1, tiles) * tile - 1)  # the last row of every tile but the last, and the next tile's first
    rows.append((n - 1) + np.arange(-3, 3))     # the last rows with values
    idx = np.unique(np.concatenate(rows))
    idx = idx[idx < padded_n - 1]
    ti = torch.from_numpy(idx.astype(np.int64)).to(DEV)
    zi = M.ints_of(host(z.index_select(0, ti)))
    zn = M.ints_of(host(z.index_select(0, ti + 1)))
    si = host(sigma.index_select(1, ti))
    live = torch.clamp(ti, max=n - 1)
    wv = [M.ints_of(host(v.index_select(0, live))) for v in vals]
    assert M.ints_of(host(z[:1])) == [1]
    for r, i in enumerate(idx.tolist()):
        w = [[wv[j][r] if i < n else 0] for j in range(4)]
        sev = [M.K[int(s) // padded_n] * pow(omega, int(s) % padded_n, M.Q) % M.Q for s in si[:, r]]
        num, den = M.factors(w, sev, 0, BETA, GAMMA, pow(omega, i, M.Q))
        assert zn[r] * den % M.Q == zi[r] * num % M.Q, i
    del z, vals
    gc.collect()
    torch.cuda.empty_cache()
    ev = engine.sigma_evaluations(sigma)
    pos = np.unique(np.concatenate([rng.integers(0, 4 * padded_n, size=20000), np.arange(n - 2, n + 70_000),
                                    np.arange(padded_n - 70_000, padded_n)]))
    tp = torch.from_numpy(pos.astype(np.int64)).to(DEV)
    got = host(ev.view(-1, 4).index_select(0, tp))
    sv = host(sigma.view(-1).index_select(0, tp))
    exp = [M.K[int(s) // padded_n] * pow(omega, int(s) % padded_n, M.Q) % M.Q for s in sv]
    assert np.array_equal(got, M.limbs_of(exp))
    pad = pos[(pos >= n) & (pos < padded_n)]
    assert len(pad) > 100_000 and all(int(s) == int(p) for s, p in zip(sv[np.searchsorted(pos, pad)], pad))
    comp.close()
    del comp, sigma, ev
    gc.collect()
    torch.cuda.empty_cache()
