"""GPU: range_check with one public (min, max) pair PER ITEM -- pg_range_check_ragged_{plan,batch,values_batch} and
pg_composer_range_check_ragged_batch -- against the CPU oracle's composer looped the reference's way,
`range_check(composer, min_i, max_i, AllocatedScalar::allocate(composer, w_i))` per item.  Every comparison is exact equality.

Items are independent and the numbering starts at (3, 5) on both sides, so ONE oracle run over the longest batch of a family of
inputs serves every shorter batch: a batch of k items is the first k items' rows and Variables."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth

pytestmark = pytest.mark.gpu

COLS = ("q_m", "q_l", "q_r", "q_o", "q_c", "w_l", "w_r", "w_o", "var_values")
ROWS = COLS[:8]
Q = synth.Q
S = pg.BlsScalar.from_int
W = 32  # RangeBoundsGD::W, the tile of the new policy (csrc/range_gadgets.hpp: PG_RC_W, as RangeCheckGD)
CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def F(x):
    from oracle import pyoracle as po
    return po.fr(synth.mont(x % Q))


# ---- shared inputs --------------------------------------------------------------------------------------------------------------
# upper bounds: the extremes interleaved, so that the ladder lengths 2 ... 255 meet inside the first tile (max = 0: max - 1 = q - 1)
_POWERS = [p for k in (3, 5, 8, 31, 63, 100, 127, 200, 252) for p in ((1 << k) - 1, 1 << k, (1 << k) + 1)]
_SHORT, _LONG = [0, 1, 2, 3, 4] + _POWERS[:13], [Q - 1, (1 << 253) + 5, (1 << 128) - 1, 1 << 64] + _POWERS[13:]
MAXES = [x for pair in zip(_SHORT, _LONG) for x in pair]
assert len(MAXES) == 36


def varied(batch, seed=1):
    """(mins, maxs, wits) as canonical integers: max from MAXES; min one of 0, 1, max - 1, max, max + 1, q - 1, random; every
    other witness inside [min, max) where that is an interval, of the rest half the edges min - 1, min, max - 1, max and half
    uniform field elements"""
    rnd = [int.from_bytes(synth.splitmix64(4, seed * 1000 + i).tobytes(), "little") % Q for i in range(2 * batch)]
    mins, maxs, wits = [], [], []
    for i in range(batch):
        mx = MAXES[i % len(MAXES)]
        mn = [0, 1, mx - 1, mx, mx + 1, Q - 1, rnd[i] % (mx + 1)][(3 * i + i // len(MAXES)) % 7] % Q
        r = rnd[batch + i]
        if i % 2 == 0:
            w = mn + r % (mx - mn) if mn < mx else r
        else:
            w = [mn - 1, mn, mx - 1, mx][(i % 16) // 2] if i % 16 < 8 else r
        mins.append(mn)
        maxs.append(mx)
        wits.append(w % Q)
    return mins, maxs, wits


def small_bounds(batch, seed):
    """bounds of 1 ... 12 bits (short items: many of them for little memory), min below, at and above max"""
    a, b = synth.splitmix64(batch, seed), synth.splitmix64(batch, seed + 1)
    maxs = [1 + int(x) % 4000 for x in a]
    mins = [int(y) % (m + 2) for y, m in zip(b, maxs)]
    wits = [int(x) % Q for x in synth.splitmix64(batch, seed + 2)]
    c = synth.splitmix64(batch, seed + 3)
    for i in range(0, batch, 2):
        if mins[i] < maxs[i]:
            wits[i] = mins[i] + int(c[i]) % (maxs[i] - mins[i])
    return mins, maxs, wits


def arrays(mins, maxs, wits):
    return synth.scalars_from_ints(mins), synth.scalars_from_ints(maxs), synth.scalars_from_ints(wits)


def oracle_loop(mins, maxs, wits):
    """the reference's loop on the oracle's composer -> its columns from (3, 5), the results, the ladder lengths and the prefix
    sums of rows / Variables per item"""
    from oracle import pyoracle as po
    from oracle.model import num_bits_closest_power_of_two
    c = po.Composer()
    assert (c.n, c.num_vars) == (3, 5)
    res, roff, voff = [], [0], [0]
    for mn, mx, w in zip(mins, maxs, wits):
        res.append(int(c.L.range_check(c.c, F(mn), F(mx), c.allocate(synth.mont(w)))))
        roff.append(c.n - 3)
        voff.append(c.num_vars - 5)
    assert c.check() == -1
    out = c.export(3, 5)
    nb = [num_bits_closest_power_of_two((mx - 1) % Q) for mx in maxs]
    assert all(r1 - r0 == 4 * n + 11 and v1 - v0 == 2 * n + 524 for r0, r1, v0, v1, n in zip(roff, roff[1:], voff, voff[1:], nb))
    out.update(result_vars=np.array(res, dtype=np.uint64), num_bits=nb, roff=roff, voff=voff)
    return out


def prefix(ora, k):
    """the oracle's answer for the first k items"""
    r, v = ora["roff"][k], ora["voff"][k]
    out = {n: ora[n][:r] for n in ROWS}
    out.update(var_values=ora["var_values"][:v], result_vars=ora["result_vars"][:k], num_bits=ora["num_bits"][:k], n_gates=r, n_vars=v)
    return out


@functools.lru_cache(maxsize=None)
def varied_oracle():
    mins, maxs, wits = varied(2 * W + 6)
    return (mins, maxs, wits), oracle_loop(mins, maxs, wits)


@functools.lru_cache(maxsize=None)
def small_oracle():
    mins, maxs, wits = small_bounds(1025, 61)
    return (mins, maxs, wits), oracle_loop(mins, maxs, wits)


def assert_cols(got, exp, names=COLS):
    for k in names:
        a, b = got[k], exp[k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)[0]
            raise AssertionError(f"{k} differs first at {bad.tolist()}: gpu={a[tuple(bad)]:#x} oracle={b[tuple(bad)]:#x}")


def emit_and_compare(engine, inputs, ora, k):
    mn, mx, wt = (a[:k] for a in arrays(*inputs))
    exp = prefix(ora, k)
    cols, res, nb, lay = engine.range_check_ragged_batch(dev(mn), dev(mx), dev(wt), 3, 5)
    torch.cuda.synchronize()
    assert (lay.n_gates, lay.n_vars) == (exp["n_gates"], exp["n_vars"])
    assert nb.cpu().numpy().tolist() == exp["num_bits"]
    assert_cols(cols.to_numpy(), exp)
    assert np.array_equal(u64(res), exp["result_vars"])
    assert engine.check_rows(cols, var_base=5) == -1
    return cols


# ---- 1. emission against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, W - 1, W, W + 1, 2 * W + 6])
def test_emission_against_the_oracle(engine, batch):
    inputs, ora = varied_oracle()
    assert {2, 255} <= set(ora["num_bits"][:W]) and len(set(ora["num_bits"][:W])) > 10  # really ragged, inside one tile
    emit_and_compare(engine, inputs, ora, batch)


# ---- 2. ragged equals uniform ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mn,mx,n", [(1, 4, 3), (0, 1 << 254, 255)])
def test_ragged_equals_uniform(engine, mn, mx, n):
    batch = W + 1
    assert engine.range_check_layout(S(mn), S(mx), batch).num_bits == n
    inside = [mn + int(x) % (mx - mn) for x in synth.splitmix64(batch, n)]
    wit = synth.random_scalars(batch, n + 1)
    wit[::2] = synth.scalars_from_ints(inside)[::2]
    wit[1], wit[3], wit[5], wit[7] = synth.scalars_from_ints([(mn - 1) % Q, mn, mx - 1, mx])
    uni, ures = engine.range_check_batch(S(mn), S(mx), dev(wit), 3, 5)
    rag, rres, nb, lay = engine.range_check_ragged_batch(dev(synth.scalars_from_ints([mn] * batch)), dev(synth.scalars_from_ints([mx] * batch)),
                                                         dev(wit), 3, 5)
    torch.cuda.synchronize()
    assert nb.cpu().numpy().tolist() == [n] * batch
    for k in COLS:
        assert torch.equal(getattr(uni, k), getattr(rag, k)), k
    assert torch.equal(ures, rres)


# ---- 3. values-only refresh (the two-block ragged region sweep) -----------------------------------------------------------------
@pytest.mark.parametrize("batch,shift", [(W + 1, 0), (2 * W + 6, 0), (2 * W + 6, 1), (2 * W + 6, 2), (2 * W + 6, 3)])
def test_values_only_refresh(engine, batch, shift):
    """the assignments alone under the plan of the bounds == var_values of the full emission (== the oracle's), the table starting
    0 / 32 / 64 / 96 bytes into a 128-byte line, canaries on both sides"""
    inputs, ora = varied_oracle()
    mn, mx, wt = (dev(a[:batch]) for a in arrays(*inputs))
    exp = prefix(ora, batch)
    nb, roff, voff = engine.ragged_buffers(batch)
    lay = engine.range_check_ragged_plan(mx, nb, roff, voff)
    assert (lay.n_gates, lay.n_vars) == (exp["n_gates"], exp["n_vars"])
    assert roff.cpu().tolist() == ora["roff"][:batch + 1] and voff.cpu().tolist() == ora["voff"][:batch + 1]
    buf = torch.full((lay.n_vars + 128 + shift, 4), CANARY, dtype=torch.int64, device="cuda:0")
    table = buf[64 + shift:64 + shift + lay.n_vars]
    engine.range_check_ragged_values(mn, mx, wt, nb, roff, voff, table)
    torch.cuda.synchronize()
    assert bool((buf[:64 + shift] == CANARY).all()) and bool((buf[64 + shift + lay.n_vars:] == CANARY).all()), "a store outside the table"
    assert np.array_equal(u64(table), exp["var_values"])
    # ... and the full emission under the same plan writes the same table
    cols = pg.Columns.allocate(lay.n_gates, lay.n_vars, "cuda:0", 3, 5)
    engine.range_check_ragged_emit(mn, mx, wt, nb, roff, voff, cols, None, 3, 5)
    torch.cuda.synchronize()
    assert torch.equal(cols.var_values, table)
    # the asynchronous plan leaves the same prefix sums and totals
    nb2, roff2, voff2 = engine.ragged_buffers(batch)
    engine.range_check_ragged_plan_async(mx, nb2, roff2, voff2)
    torch.cuda.synchronize()
    assert torch.equal(nb, nb2) and torch.equal(roff, roff2) and torch.equal(voff, voff2)
    assert engine.plan_result()[0].n_gates == lay.n_gates


# ---- 4. both homes of the inverses (csrc/invert.hpp: 2^11 and 2^18 inverted elements, two per item) -----------------------------
@pytest.mark.parametrize("batch", [1023, 1024, 1025])
def test_around_the_lower_threshold_against_the_oracle(engine, batch):
    inputs, ora = small_oracle()
    emit_and_compare(engine, inputs, ora, batch)


def test_across_the_upper_threshold(engine):
    """2^17 - 1 items (inverses written in place beside the emitter) against 2^17 of the same inputs (dense, pre-pass first):
    the common prefix agrees byte for byte, and both satisfy every gate"""
    n_big = 1 << 17
    mn, mx, wt = (dev(a) for a in arrays(*small_bounds(n_big, 71)))
    outs = []
    for n in (n_big - 1, n_big):
        cols, res, nb, lay = engine.range_check_ragged_batch(mn[:n], mx[:n], wt[:n], 3, 5)
        torch.cuda.synchronize()
        assert engine.check_rows(cols, var_base=5) == -1
        outs.append((cols, res))
    rows, nv = int(outs[0][0].q_m.shape[0]), int(outs[0][0].var_values.shape[0])
    for k in ROWS:
        assert torch.equal(getattr(outs[0][0], k), getattr(outs[1][0], k)[:rows]), k
    assert torch.equal(outs[0][0].var_values, outs[1][0].var_values[:nv])
    assert torch.equal(outs[0][1], outs[1][1][:n_big - 1])


# ---- 5. on the composer ---------------------------------------------------------------------------------------------------------
def same(devc, ora):
    got, exp = devc.export(), ora.export()
    assert devc.circuit_size() == ora.n and devc.num_variables() == ora.num_vars
    assert_cols(got, exp)


def oracle_value(ora, var):
    from oracle import pyoracle as po
    return po.fr_to_int(ora.L.composer_value(ora.c, var))


@pytest.mark.parametrize("items", [5, 40])
def test_on_the_composer(engine, items):
    """add_input_batch, a uniform range_check_batch, the new call, max_bound_ragged_batch, and the results constrained to what the
    oracle expects: export, check, sigma at two domain sizes, materialize, the grand product -- with 5 items (below
    kFootprintMinRows) and with enough items for a footprint of the call's own"""
    from oracle import pyoracle as po
    mins, maxs, wits = varied(items, seed=2)
    mn, mx, wt = arrays(mins, maxs, wits)
    devc, ora = pg.StandardComposer(engine, 1 << 16, 1 << 16), po.Composer()
    L = ora.L
    extra = synth.random_scalars(4, 9)
    first = devc.add_input_batch(dev(extra))
    assert first == [ora.add_input(x) for x in extra][0]
    uw = [60_000, 7, 250_000, 123_456]
    r0 = devc.range_check_batch(S(50_000), S(250_000), dev(synth.scalars_from_ints(uw)))
    o0 = [int(L.range_check(ora.c, F(50_000), F(250_000), ora.allocate(synth.mont(w)))) for w in uw]
    n_before = devc.circuit_size()
    r1, nb = devc.range_check_ragged_batch(dev(mn), dev(mx), dev(wt))
    o1 = [int(L.range_check(ora.c, F(a), F(b), ora.allocate(synth.mont(w)))) for a, b, w in zip(mins, maxs, wits)]
    assert (devc.circuit_size() - n_before >= 4096) == (items > 5)
    n_out = C.c_uint64()
    r2, _ = devc.max_bound_ragged_batch(dev(mx), dev(wt))
    o2 = [int(L.max_bound(ora.c, F(b), ora.allocate(synth.mont(w)), C.byref(n_out))) for b, w in zip(maxs, wits)]
    assert [u64(r).tolist() for r in (r0, r1, r2)] == [o0, o1, o2]
    from oracle.model import num_bits_closest_power_of_two
    assert nb.cpu().numpy().tolist() == [num_bits_closest_power_of_two((b - 1) % Q) for b in maxs]
    results = o0 + o1 + o2
    values = [oracle_value(ora, r) for r in results]
    assert set(values) == {0, 1}
    for want in (1, 0):
        vs = [r for r, v in zip(results, values) if v == want]
        devc.constrain_to_constant_batch(torch.tensor(vs, dtype=torch.int64, device="cuda:0"), S(want))
        for r in vs:
            L.composer_constrain_to_constant(ora.c, r, F(want), None)
    same(devc, ora)
    assert devc.check() == -1 and ora.check() == -1
    n = devc.circuit_size()
    padded = 1 << (n - 1).bit_length()
    for p in (padded, 2 * padded):
        assert np.array_equal(u64(devc.permutation(p)), ora.sigma(p)), p
    m, full, exp = devc.materialize(), ora.full_columns(), ora.export()
    for k in ("q_4", "q_arith"):
        assert np.array_equal(u64(m[k]), full[k]), k
    for k in ("q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add"):
        assert int(m[k].abs().sum()) == 0, k
    assert np.array_equal(u64(m["w_4"]), full["w_4"])
    for wname, wire in (("w_l", exp["w_l"]), ("w_r", exp["w_r"]), ("w_o", exp["w_o"]), ("w_4", full["w_4"])):
        assert np.array_equal(u64(m[wname + "_value"]), exp["var_values"][wire.astype(np.int64)]), wname
    assert devc.copy_constraints_hold()
    devc.close()


# ---- 6. clear_witness -----------------------------------------------------------------------------------------------------------
def test_clear_witness_finds_the_call_in_place(engine):
    """the same bounds and other witnesses: the call's rows are found in place (a bent limb survives) and only var_values changes;
    one bound changed -- a min, then a max -- is another circuit: what precedes the call stays, the call is emitted again"""
    from oracle import pyoracle as po
    mins, maxs, _ = varied(12, seed=3)
    uw = [60_000, 7, 250_000]

    def build(devc, ora, seed, mins, maxs):
        wits = varied(12, seed=seed)[2]
        r0 = devc.range_check_batch(S(50_000), S(250_000), dev(synth.scalars_from_ints([w + seed for w in uw])))
        o0 = [int(ora.L.range_check(ora.c, F(50_000), F(250_000), ora.allocate(synth.mont(w + seed)))) for w in uw]
        r1, _ = devc.range_check_ragged_batch(*(dev(a) for a in arrays(mins, maxs, wits)))
        o1 = [int(ora.L.range_check(ora.c, F(a), F(b), ora.allocate(synth.mont(w)))) for a, b, w in zip(mins, maxs, wits)]
        assert u64(r0).tolist() == o0 and u64(r1).tolist() == o1
        devc.boolean_gate_batch(r1)
        for r in o1:
            ora.L.composer_boolean_gate(ora.c, r)

    devc, ora = pg.StandardComposer(engine, 1 << 14, 1 << 14), po.Composer()
    build(devc, ora, 4, mins, maxs)
    same(devc, ora)
    n1, first = devc.circuit_size(), devc.export()
    before = engine.range_check_layout(S(50_000), S(250_000), 3).n_gates  # rows of the uniform call
    row = 3 + before + 5  # a row of the ragged call
    cols = devc.device_columns()
    cols.q_o[row, 1] ^= 0x55
    torch.cuda.synchronize()
    devc.clear_witness()
    ora = po.Composer()
    build(devc, ora, 5, mins, maxs)
    assert devc.refresh_stats() == (n1 - 3, 0, True)
    got = devc.export()
    assert got["q_o"][row, 1] == first["q_o"][row, 1] ^ np.uint64(0x55), "a row found in place was written again"
    cols = devc.device_columns()
    cols.q_o[row, 1] ^= 0x55
    torch.cuda.synchronize()
    got = devc.export()
    for k in ROWS:
        assert np.array_equal(got[k], first[k]), k
    assert not np.array_equal(got["var_values"], first["var_values"])
    same(devc, ora)  # == a fresh build on the second witnesses
    assert devc.check() == ora.check() == -1
    for which in ("min", "max"):
        m2, x2 = list(mins), list(maxs)
        if which == "min":
            m2[7] = (m2[7] + 1) % Q
        else:
            x2[7] = (x2[7] + 1) % Q
        devc.clear_witness()
        ora = po.Composer()
        build(devc, ora, 6, m2, x2)
        kept, rewritten, refreshing = devc.refresh_stats()
        assert not refreshing and kept == before and rewritten > 0, (which, kept, rewritten)
        same(devc, ora)
        assert devc.check() == ora.check() == -1
        # back to the first bounds: this build's log holds the changed call, so again only the uniform call is found
        devc.clear_witness()
        ora = po.Composer()
        build(devc, ora, 7, mins, maxs)
        assert devc.refresh_stats()[0] == before
        same(devc, ora)
    devc.close()


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------
def test_prove_and_verify(engine):
    """a handful of ragged items, their results constrained to the expected 0 / 1: the proof under a development key is accepted;
    with one expected constant flipped it is rejected"""
    tau = S(0x5EED_7A0 ** 9 % Q)
    ck = pg.CommitKey.setup(engine, 1 << 12, tau)
    ok = pg.OpeningKey.setup(engine, tau)
    mins = [0, 50_000, 5, 7, 100, 0]
    maxs = [16, 250_000, 5, 3, 200, 1 << 20]
    wits = [15, 250_000, 5, 8, 150, (1 << 20) - 1]
    want = [1, 0, 0, 0, 1, 1]
    assert want == [int(a <= w < b) for a, b, w in zip(mins, maxs, wits)]
    verdicts = []
    for flip in (None, 2):
        comp = pg.StandardComposer(engine, 1 << 11, 1 << 13)
        res, _ = comp.range_check_ragged_batch(*(dev(a) for a in arrays(mins, maxs, wits)))
        for i, r in enumerate(u64(res).tolist()):
            comp.constrain_to_constant(r, S(want[i] ^ (i == flip)), None)
        comp.sync()
        assert comp.circuit_size() <= 1 << 11
        assert (comp.check() == -1) == (flip is None)
        proof = comp.prove(ck, b"plonk")
        verdicts.append(proof.verify(comp.verifier_key(ck), ok, {}))
        comp.close()
    ok.close()
    assert verdicts == [True, False]


# ---- 8. edges -------------------------------------------------------------------------------------------------------------------
def test_edges(engine):
    from plonk_gadgets_amd import _lib
    lib = _lib.load()
    comp = pg.StandardComposer(engine, 1 << 10, 1 << 12)
    empty = torch.empty((0, 4), dtype=torch.int64, device="cuda:0")
    res, nb = comp.range_check_ragged_batch(empty, empty, empty)
    assert res.numel() == 0 and nb.numel() == 0 and (comp.circuit_size(), comp.num_variables()) == (3, 5)
    cols, res, nb, lay = engine.range_check_ragged_batch(empty, empty, empty, 3, 5)
    assert (lay.n_gates, lay.n_vars) == (0, 0) and res.numel() == 0
    a3, a4 = dev(synth.scalars_from_ints([1, 2, 3])), dev(synth.scalars_from_ints([1, 2, 3, 4]))
    for bad in ((a3, a4, a4), (a4, a3, a4), (a4, a4, a3)):
        with pytest.raises(ValueError):
            comp.range_check_ragged_batch(*bad)
        with pytest.raises(ValueError):
            engine.range_check_ragged_batch(*bad)
    assert (comp.circuit_size(), comp.num_variables()) == (3, 5)
    # NULL arrays: PG_ERR_INVALID_ARGUMENT (2), nothing appended
    nbt, roff, voff = engine.ragged_buffers(4)
    lay = engine.range_check_ragged_plan(a4, nbt, roff, voff)
    out = pg.Columns.allocate(lay.n_gates, lay.n_vars, "cuda:0", 3, 5)
    cc, st, p = out.as_c(), engine._stream(), a4.data_ptr()
    n, r, v = nbt.data_ptr(), roff.data_ptr(), voff.data_ptr()
    layc = _lib.LayoutC()
    for args in ((None, 4, n, r, v), (p, 4, None, r, v), (p, 4, n, None, v), (p, 4, n, r, None)):
        assert lib.pg_range_check_ragged_plan(engine._h, *args, C.byref(layc), st) == 2
        assert lib.pg_range_check_ragged_plan_async(engine._h, *args, st) == 2
    assert lib.pg_range_check_ragged_plan(engine._h, p, 4, n, r, v, None, st) == 2
    for args in ((None, p, p, 4, n, r, v), (p, None, p, 4, n, r, v), (p, p, None, 4, n, r, v), (p, p, p, 4, None, r, v),
                 (p, p, p, 4, n, None, v), (p, p, p, 4, n, r, None)):
        assert lib.pg_range_check_ragged_batch(engine._h, *args, 3, 5, C.byref(cc), None, st) == 2
        assert lib.pg_range_check_ragged_values_batch(engine._h, *args, out.var_values.data_ptr(), st) == 2
    assert lib.pg_range_check_ragged_batch(engine._h, p, p, p, 4, n, r, v, 3, 5, None, None, st) == 2
    assert lib.pg_range_check_ragged_values_batch(engine._h, p, p, p, 4, n, r, v, None, st) == 2
    assert lib.pg_range_check_ragged_batch(None, p, p, p, 4, n, r, v, 3, 5, C.byref(cc), None, st) == 2
    rv = torch.empty((4,), dtype=torch.int64, device="cuda:0")
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.pg_composer_range_check_ragged_batch(comp._h, *args, 4, rv.data_ptr(), None) == 2
        assert (comp.circuit_size(), comp.num_variables()) == (3, 5)
    assert lib.pg_composer_range_check_ragged_batch(None, p, p, p, 4, rv.data_ptr(), None) == 2
    # ... and the composer still works: result Variables and ladder lengths may both be left out
    assert lib.pg_composer_range_check_ragged_batch(comp._h, p, p, p, 4, None, None) == 0
    assert comp.check() == -1 and comp.circuit_size() > 3
    comp.close()
