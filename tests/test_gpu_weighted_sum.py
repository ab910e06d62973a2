"""GPU: weighted_sum_ragged_batch on the device composer against the loop of composer.add calls it stands for,
replayed on the C oracle's composer (tests/weighted_sum_oracle.py), through tests/widget_programs.assert_device_equals_oracle: the
nine columns, var_values, check(), wire values, sigma at n and padded, the sparse list's second pass.  Shapes come from
pg_weighted_sum_geometry (T terms a tile, P tiles a carry pass): the cases of tests/test_weighted_sum_model.py, where the call
stands and what its terms are, every tile edge, the carry launch's pass boundary (too long to replay: the closed form, check(),
Python-integer sums and a bumped input), the witness refresh, the refused calls, a stream that is behind, and random programs."""
import ctypes as C
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch

import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth
from tests import weighted_sum_model as wm
from tests import weighted_sum_oracle as wso
from tests import weighted_sum_programs as wprog
from tests.widget_programs import assert_device_equals_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lagging_stream import LATE, lagging, release  # noqa: E402

R = wm.R
S = pg.BlsScalar.from_int
CASES = wso.cases()
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c")


def geometry():
    from plonk_gadgets_amd import _lib
    t, p = C.c_uint32(), C.c_uint32()
    assert _lib.load().pg_weighted_sum_geometry(C.byref(t), C.byref(p)) == 0
    return int(t.value), int(p.value)


T, P = geometry()


@pytest.fixture(scope="module")
def engine():
    e = pg.Engine(0)
    yield e
    e.close()


def composer(engine, cap=1 << 14):
    dev = pg.StandardComposer(engine, cap, cap)
    dev.auto_grow()
    return dev


def tv(xs):
    return torch.tensor([int(x) for x in xs], dtype=torch.int64, device="cuda")


def dev_scalars(vals):
    return torch.from_numpy(synth.scalars_from_ints([v % R for v in vals]).view(np.int64)).cuda()


def u64(a):
    return np.ascontiguousarray(np.asarray(a)).view(np.uint64)


# ---- 1. against the oracle, everything ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cpu_cases_against_the_oracle(engine, case):
    both = wso.Both(composer(engine))
    wso.run_case(both, case)
    assert_device_equals_oracle(both)
    both.dev.close()


def test_where_the_call_stands_and_what_its_terms_are(engine):
    """first in a composer (on the Variables it is born with) and without d_result_vars; between two footprints, on results of
    add_batch, of range_check_batch and of the earlier sum; one Variable as a term of 257 segments; results under range_gate_batch;
    and last"""
    rng = random.Random(41)
    both = wso.Both(composer(engine))
    res0 = both.weighted_sum_ragged_batch([0, 1, 2, 3, 4], [0, 2, 5], want_results=False)
    rc = both.range_check_batch(3, 200, [100, 5, 250])                                   # a footprint before
    a = both.add_input_batch([rng.randrange(1 << 12) for _ in range(12)])
    ab = both.add_batch(1, a[:6], 1, a[6:], 7)
    x = rc + ab + res0 + a[:3]
    res1 = both.weighted_sum_ragged_batch(x, [0, 3, 9, 11, len(x)], [rng.randrange(1, 6) for _ in x], [0, 5, 0, 1])
    both.conditionally_select_zero_batch(a[:5], rc + rc[:2])                             # a footprint behind
    shared = a[0]
    x = list(itertools.chain.from_iterable((shared, rng.choice(a)) for _ in range(257)))
    res2 = both.weighted_sum_ragged_batch(x, list(range(0, 515, 2)), None, None)
    # res2 < 2^13; res1[1] sums six add_batch results (< 2^13 + 7 each) with coefficients < 6 and a constant
    both.range_gate_batch(res2[:40] + [res1[1]], 20)
    both.weighted_sum_ragged_batch(res2[:7] + res1, [0, 2, 7, 11], [R - 1] * 11, [R - 1, 0, 3])   # last; sums of sums
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)
    both.dev.close()


# ---- 2. tile edges ------------------------------------------------------------------------------------------------------------
def cut(total, lo, hi, rng):
    off = [0]
    while total - off[-1] > hi + lo:
        off.append(off[-1] + rng.randrange(lo, hi + 1))
    off.append(total)
    return off


EDGES = {
    "terms_T": [0, T],
    "terms_T_minus_1": [0, T - 1],
    "terms_T_plus_1": [0, T + 1],
    "two_terms_across_the_edge": [0, T - 1, T + 1, T + 4],
    "a_segment_ends_at_the_edge": [0, 5, T, 2 * T + 1],
    "through_two_tiles_without_a_start": [0, T // 2, 3 * T + 6],
    "only_two_term_segments": list(range(0, 2 * T + 3, 2)),
    "ragged_with_a_partial_last_tile": cut(2 * T + 377, 2, T // 3, random.Random(8)),
}


@pytest.mark.parametrize("name", list(EDGES))
@pytest.mark.parametrize("optional", ("coeffs_constants", "bare"))
def test_tile_edges_against_the_oracle(engine, name, optional):
    seg_off = EDGES[name]
    rng = random.Random(len(seg_off) * 7 + (optional == "bare"))
    both = wso.Both(composer(engine))
    pool = both.add_input_batch([rng.randrange(1 << 32) for _ in range(64)])
    x = [rng.choice(pool) for _ in range(seg_off[-1])]
    co = ks = None
    if optional != "bare":
        co = [rng.choice([1, 2, 3, R - 1, rng.randrange(1 << 16)]) for _ in x]
        ks = [rng.choice([0, 1, R - 1, rng.randrange(1 << 40)]) for _ in seg_off[1:]]
    both.weighted_sum_ragged_batch(x, seg_off, co, ks)
    assert both.first_bad() == -1
    assert_device_equals_oracle(both)
    both.dev.close()


# ---- 3. carry passes ----------------------------------------------------------------------------------------------------------
LONG = (P + 1) * T + 3


@pytest.mark.parametrize("shape", ("one_segment", "ragged"))
def test_carries_across_the_pass_boundary(engine, shape):
    """(P + 1) T + 3 terms: the carry launch takes two passes.  Too long to replay on the oracle: the structure against the closed
    form, the values by check() and by Python-integer sums, and one bumped input names exactly its term's row"""
    rng = random.Random(17 + (shape == "ragged"))
    nprng = np.random.default_rng(5)
    seg_off = [0, LONG] if shape == "one_segment" else cut(LONG, 2, 3 * T, rng)
    segments = len(seg_off) - 1
    dev = pg.StandardComposer(engine, LONG + 64, LONG + 8192)
    pool_vals = [rng.randrange(1 << 62) for _ in range(4096)]
    first = dev.add_input_batch(dev_scalars(pool_vals))
    special = dev.add_input(S(12345))                       # the Variable of ONE term
    idx = nprng.integers(0, 4096, LONG)
    t_star = P * T + T // 2 + 1                             # behind the pass boundary, inside a tile
    x = first + idx
    x[t_star] = special
    co_pool = [1, 2, R - 1, R - 2] + [rng.randrange(R) for _ in range(60)]
    co_idx = nprng.integers(0, 64, LONG)
    ks = [rng.choice([0, 1, R - 1, rng.randrange(R)]) for _ in range(segments)]
    co_limbs = synth.scalars_from_ints(co_pool)[co_idx]
    n0, v0 = dev.circuit_size(), dev.num_variables()
    res = dev.weighted_sum_ragged_batch(torch.from_numpy(x).cuda(), tv(seg_off), torch.from_numpy(co_limbs.view(np.int64)).cuda(), dev_scalars(ks))
    assert dev.circuit_size() == n0 + LONG - segments and dev.num_variables() == v0 + LONG - segments
    # structure
    got = dev.export(n0, v0)
    w_l, w_r, w_o, t_of, s_of, is_first = wm.closed_form(x, seg_off, v0)
    for k, exp in (("w_l", w_l), ("w_r", w_r), ("w_o", w_o)):
        assert np.array_equal(u64(got[k]), exp.astype(np.uint64)), k
    one, neg1, zero = (np.array(synth.mont(v), dtype=np.uint64) for v in (1, R - 1, 0))
    ks_limbs = synth.scalars_from_ints(ks)
    assert not u64(got["q_m"]).any()
    assert (u64(got["q_o"]).reshape(-1, 4) == neg1).all()
    assert np.array_equal(u64(got["q_l"]).reshape(-1, 4), np.where(is_first[:, None], co_limbs[t_of - 1], one))
    assert np.array_equal(u64(got["q_r"]).reshape(-1, 4), co_limbs[t_of])
    assert np.array_equal(u64(got["q_c"]).reshape(-1, 4), np.where(is_first[:, None], ks_limbs[s_of], zero))
    assert res.cpu().tolist() == [v0 + seg_off[s + 1] - s - 2 for s in range(segments)]
    # values
    assert dev.check() == -1
    vals = pool_vals + [12345]
    p = [co_pool[c] * vals[v - first] for c, v in zip(co_idx.tolist(), x.tolist())]
    pre = [0] + list(itertools.accumulate(p))
    starts = set(seg_off[:-1])
    seg_of = np.searchsorted(np.array(seg_off), np.arange(LONG), side="right") - 1
    tiles = [0, LONG // T, P - 1, P, rng.randrange(1, P - 1), rng.randrange(1, P - 1)]
    picks = [min(tl * T + T - 1, LONG - 1) for tl in tiles] + [rng.randrange(LONG) for _ in range(1000)]
    table = u64(got["var_values"]).reshape(-1, 4)
    for t in picks:
        t += t in starts                                    # (a segment's first term owns no Variable: the one behind it)
        s = int(seg_of[t])
        assert synth.to_int(table[t - s - 1]) == (ks[s] + pre[t + 1] - pre[seg_off[s]]) % R, t
    # one bumped input: exactly its term's row
    cols = dev.device_columns()
    kept = cols.var_values[special].clone()
    cols.var_values[special, 0] += 1
    assert dev.check() == n0 + t_star - int(seg_of[t_star]) - 1
    cols.var_values[special] = kept
    assert dev.check() == -1
    del cols
    dev.close()


# ---- 4. refresh ---------------------------------------------------------------------------------------------------------------
REFRESH_OFF = cut(T + 300, 2, 40, random.Random(3))


def refresh_call(both, values, seg_off=REFRESH_OFF, coeff_at=None, constant_at=None):
    rng = random.Random(91)
    pool = both.add_input_batch(values)
    x = [rng.choice(pool) for _ in range(seg_off[-1])]
    co = [rng.choice([1, 2, R - 1, rng.randrange(R)]) for _ in x]
    ks = [rng.randrange(R) for _ in seg_off[1:]]
    if coeff_at is not None:
        co[coeff_at] = (co[coeff_at] + 1) % R
    if constant_at is not None:
        ks[constant_at] = (ks[constant_at] + 1) % R
    return both.weighted_sum_ragged_batch(x, seg_off, co, ks)


def test_clear_witness_finds_the_rows_in_place(engine):
    """the same call on other witnesses writes assignments only; with another seg_off of the same totals, one coefficient or one
    constant moved it is another call -- each against a build of the unchanged call -- and every outcome equals the oracle"""
    rng = random.Random(6)
    rows = REFRESH_OFF[-1] - (len(REFRESH_OFF) - 1)
    j = next(i for i in range(1, len(REFRESH_OFF) - 1) if REFRESH_OFF[i + 1] - REFRESH_OFF[i] >= 3)
    moved_off = list(REFRESH_OFF)
    moved_off[j] += 1                                       # the same totals, one term in another segment
    dev = composer(engine)
    for change in ({}, {"seg_off": moved_off}, {"coeff_at": T + 5}, {"constant_at": 2}):
        dev.clear_witness()
        refresh_call(wso.Both(dev), [rng.randrange(R) for _ in range(50)])      # the unchanged call (again)
        dev.clear_witness()
        both = wso.Both(dev)
        refresh_call(both, [rng.randrange(R) for _ in range(50)], **change)
        kept, rewritten, refreshing = dev.refresh_stats()
        assert (kept, rewritten, refreshing) == ((rows, 0, True) if not change else (0, rows, False)), change
        assert_device_equals_oracle(both)
    dev.close()


def test_the_values_only_call_leaves_the_rows_alone(engine):
    rng = random.Random(7)
    dev = composer(engine)
    n0 = dev.circuit_size()
    refresh_call(wso.Both(dev), [rng.randrange(R) for _ in range(50)])
    cols = dev.device_columns()
    n = dev.circuit_size()
    for k in SELECTORS + ("w_l", "w_r", "w_o"):
        getattr(cols, k)[n0:n] = -7
    del cols
    dev.clear_witness()
    second = [rng.randrange(R) for _ in range(50)]
    res = refresh_call(wso.Both(dev), second)
    assert dev.refresh_stats() == (n - n0, 0, True)
    got = dev.export(n0)
    for k in SELECTORS + ("w_l", "w_r", "w_o"):
        assert (np.asarray(got[k]).view(np.int64) == -7).all(), k
    fresh = wso.Both(composer(engine))
    assert refresh_call(fresh, second) == res
    assert np.array_equal(u64(dev.export()["var_values"]), u64(fresh.dev.export()["var_values"]))
    fresh.dev.close()
    dev.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refused_calls_append_nothing(engine):
    dev = pg.StandardComposer(engine)
    first = dev.add_input_batch(dev_scalars([1, 2, 3, 4, 5, 6]))
    state = (dev.circuit_size(), dev.num_variables())
    x, off = tv(range(first, first + 6)), tv([0, 2, 4, 6])
    co, ks = dev_scalars([1, 2, 3, 4, 5, 6]), dev_scalars([7, 8, 9])
    raw_r = torch.from_numpy(np.array([R >> (64 * j) & (2**64 - 1) for j in range(4)], dtype=np.uint64).view(np.int64)).cuda()

    def refused(match, *args):
        with pytest.raises(pg.PgError, match=match) as e:
            dev.weighted_sum_ragged_batch(*args)
        assert e.value.status == 2
        assert (dev.circuit_size(), dev.num_variables()) == state

    refused("unknown Variable", tv([first, dev.num_variables(), first, first, first, first]), off, co, ks)
    refused(r"first offending segment is 0\b", x, tv([1, 2, 4, 6]), co, ks)
    refused(r"first offending segment is 2\b", x, tv([0, 2, 4, 5]), co, ks)          # the last entry is not terms
    refused(r"first offending segment is 2\b", x, tv([0, 2, 4, 1 << 40]), co, ks)    # ... and far beyond: refused, not used
    refused(r"first offending segment is 2\b", x, tv([0, 2, 1 << 40, 6]), co, ks)
    refused(r"first offending segment is 1\b", x, tv([0, 2, 3, 6]), co, ks)          # a 1-term segment in the middle
    refused(r"first offending segment is 1\b", x, tv([0, 4, 2, 6]), co, ks)          # a decreasing pair
    refused(r"first offending segment is 0\b", x, tv([0, 0, 4, 6]), None, None)      # an empty segment
    bad_co, bad_ks = co.clone(), ks.clone()
    bad_co[3], bad_co[5], bad_ks[1] = raw_r, raw_r, raw_r
    refused(r"coefficient 3\b", x, off, bad_co, ks)
    refused(r"constant 1\b", x, off, co, bad_ks)
    refused("no segment", x, tv([0]), None, None)
    for args in ((x, off, co[:5], ks), (x, off, co, ks[:2]), (x, off[:0], None, None)):
        with pytest.raises(ValueError):
            dev.weighted_sum_ragged_batch(*args)
    lib = dev._lib
    call = lib.pg_composer_weighted_sum_ragged_batch
    assert call(None, x.data_ptr(), off.data_ptr(), None, None, 6, 3, None) == 2
    assert call(dev._h, None, off.data_ptr(), None, None, 6, 3, None) == 2
    assert call(dev._h, x.data_ptr(), None, None, None, 6, 3, None) == 2
    assert call(dev._h, x.data_ptr(), off.data_ptr(), None, None, 1 << 32, 3, None) == 2
    assert (dev.circuit_size(), dev.num_variables()) == state and dev.check() == -1
    # no segments: nothing, and PG_OK
    assert dev.weighted_sum_ragged_batch(x[:0], tv([0])).shape == (0,)
    assert (dev.circuit_size(), dev.num_variables()) == state
    # and the composer still works
    res = dev.weighted_sum_ragged_batch(x, off, co, ks)
    assert res.cpu().tolist() == [state[1], state[1] + 1, state[1] + 2] and dev.check() == -1
    assert synth.to_int(u64(dev.export()["var_values"]).reshape(-1, 4)[state[1] + 2]) == 9 + 5 * 5 + 6 * 6
    dev.close()


# ---- 6. stream order ----------------------------------------------------------------------------------------------------------
def test_weighted_sum_under_a_lagging_stream(engine):
    """a composer made on the default stream; the four arrays are filled in on a side stream that is behind: while the host issues
    the call they hold other Variables, other (valid) offsets, other coefficients and other constants"""
    rng = random.Random(79)
    side = torch.cuda.Stream()
    seg_off = cut(T + 200, 2, 30, rng)
    terms, segments = seg_off[-1], len(seg_off) - 1
    values = [rng.randrange(R) for _ in range(64)]
    idx = [rng.randrange(32) for _ in range(terms)]
    co = [rng.randrange(R) for _ in range(terms)]
    ks = [rng.randrange(R) for _ in range(segments)]
    stale_off = list(range(0, 2 * segments, 2)) + [terms]         # as many segments, other boundaries

    def fill(c):
        return c.add_input_batch(dev_scalars(values))

    comp = pg.StandardComposer(engine, 1 << 12, 1 << 13)
    first = fill(comp)
    t_x, t_off, t_co, t_ks = tv([first + i for i in idx]), tv(seg_off), dev_scalars(co), dev_scalars(ks)
    b_x, b_off = tv([first + 32 + i for i in idx]), tv(stale_off)
    b_co, b_ks = dev_scalars([c ^ 1 for c in co]), dev_scalars([k ^ 1 for k in ks])
    c0 = pg.StandardComposer(engine, 1 << 12, 1 << 13)            # warm-up on another composer, under both streams
    fill(c0)
    c0.weighted_sum_ragged_batch(b_x, b_off, b_co, b_ks)
    with torch.cuda.stream(side):
        c0.weighted_sum_ragged_batch(b_x, b_off, b_co, b_ks)
    c0.sync()
    c0.close()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            ev = lagging(side)
            b_x.copy_(t_x)
            b_off.copy_(t_off)
            b_co.copy_(t_co)
            b_ks.copy_(t_ks)
            assert not ev.query(), LATE
            res = comp.weighted_sum_ragged_batch(b_x, b_off, b_co, b_ks)    # (it checks its arrays first: a host synchronisation)
            got_check = comp.check()
        torch.cuda.synchronize()
        both = wso.Both(None)
        pool = both.add_input_batch(values)
        exp = both.weighted_sum_ragged_batch([pool[i] for i in idx], seg_off, co, ks)
        assert res.cpu().tolist() == exp and got_check == -1
        got, want = comp.export(), both.ora.export()
        for k in want:
            assert np.array_equal(u64(got[k]).reshape(-1), u64(want[k]).reshape(-1)), k
    finally:
        release()
        comp.close()


# ---- 7. random programs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", wprog.SEEDS)
def test_random_programs(engine, seed):
    both = wprog.run_program(composer(engine), seed)
    try:
        assert_device_equals_oracle(both)
    except AssertionError as e:
        raise AssertionError(f"seed {seed}, program {[c[:3] for c in both.log]}: {e}")
    both.dev.close()


# ---- 8. the signature among its neighbours ------------------------------------------------------------------------------------
def test_the_signature_tells_the_call_from_its_neighbours(engine):
    """what tests/test_gpu_clear_witness.py's table asks of every batched append, for this one and the call most like it -- an
    add_batch of as many rows at the same place: the SAME call on other witnesses finds its rows in place; the OTHER call there finds
    nothing in place, ends the refresh and leaves the composer a fresh build of it would be"""
    co, ks = dev_scalars([3, R - 1, 1, 0, 5, 2]), dev_scalars([9, 0, R - 1])

    def inputs(dev, seed):
        rng = random.Random(seed)
        return dev.add_input_batch(dev_scalars([rng.randrange(R) for _ in range(8)]))

    def wsum(dev, first):
        dev.weighted_sum_ragged_batch(tv([first, first + 1, first + 2, first + 3, first + 4, first + 1]), tv([0, 2, 4, 6]), co, ks)

    def adds(dev, first):
        dev.add_batch(S(3), tv([first, first + 2, first + 4]), S(R - 1), tv([first + 1, first + 3, first + 1]), S(9))

    for call, other in ((wsum, adds), (adds, wsum)):
        dev = composer(engine)
        call(dev, inputs(dev, 1))
        rows = dev.circuit_size() - 3
        assert rows == 3
        dev.clear_witness()
        call(dev, inputs(dev, 2))
        assert dev.refresh_stats() == (rows, 0, True)
        dev.clear_witness()
        other(dev, inputs(dev, 3))
        assert dev.refresh_stats() == (0, rows, False)
        fresh = composer(engine)
        other(fresh, inputs(fresh, 3))
        got, want = dev.export(), fresh.export()
        for k in want:
            assert np.array_equal(u64(got[k]), u64(want[k])), k
        assert dev.check() == -1
        fresh.close()
        dev.close()
