#!/usr/bin/env python3
"""A circuit built, checked and made prover-ready without leaving the GPU.

    python examples/circuit_on_device.py [log2_witnesses]

The reference's loop
    for w in witnesses { let a = AllocatedScalar::allocate(composer, w); results.push(range_check(composer, min, max, a)); }
is one batched append on the device-resident composer; single calls with the reference's signatures mix in freely.  Then a
per-account limit check: every amount in 16 bits, limit - (the account's amounts) by ONE weighted_sum_ragged_batch over ragged
accounts, and the headrooms in 16 bits again.  Last, a small circuit of its own that is proven and verified: min(x, y) of pairs of
64-bit amounts, from the bit [x <= y] (is_less_equal_each) and gate batches.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonk_gadgets_amd as pg
from plonk_gadgets_amd import synth


def main():
    lg = int(sys.argv[1]) if len(sys.argv) > 1 else 14
    batch = 1 << lg
    S = pg.BlsScalar.from_int
    engine = pg.Engine(0)
    composer = pg.StandardComposer(engine)
    composer.auto_grow()                                   # grow like the reference's Vecs ...
    lay = engine.range_check_layout(S(0), S(2**254), batch)
    composer.reserve(lay.n_gates + 64, lay.n_vars + 64)    # ... but the big append's size is known: make room once

    # witnesses arrive as canonical little-endian bytes (BlsScalar::to_bytes): convert in bulk on the device
    canonical = torch.from_numpy(synth.splitmix64(4 * batch, 1).reshape(batch, 4).copy().view(np.int64)).to("cuda:0")
    canonical[:, 3] &= (1 << 60) - 1                       # keep them below q
    witnesses, _, bad = engine.scalars_from_canonical(canonical)
    assert bad == 0

    t = time.perf_counter()
    results = composer.range_check_batch(S(0), S(2**254), witnesses)          # allocate + range_check, per witness
    first = pg.AllocatedScalar.allocate(composer, S(7))                       # single calls, reference signatures
    inside = pg.range_check(composer, S(5), S(10), first)
    both = pg.conditionally_select_zero(composer, inside, int(results[0]))    # inside AND first batched result
    composer.constrain_to_constant(both, S(1), None)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t
    n = composer.circuit_size()
    assert composer.check() == -1                          # every row satisfies its gate equation
    built_rows = n

    # amounts against per-account limits: accounts of 2 .. 9 transfers of < 2^12 each, every limit 2^16 - 1
    accounts = max(1, batch // 8)
    sizes = torch.randint(2, 10, (accounts,), device="cuda:0")
    seg_off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(sizes, 0)])
    transfers = int(seg_off[-1])
    small = lambda xs: torch.from_numpy(synth.scalars_from_ints(xs).view(np.int64)).to("cuda:0")
    amounts = small(range(1 << 12))[torch.randint(0, 1 << 12, (transfers,), device="cuda:0")].contiguous()
    first_amount = composer.add_input_batch(amounts)
    amount_vars = torch.arange(first_amount, first_amount + transfers, dtype=torch.int64, device="cuda:0")
    composer.range_gate_batch(amount_vars, 16)                                   # every amount < 2^16
    minus_one, limit = small([synth.Q - 1]), small([2**16 - 1])
    headroom = composer.weighted_sum_ragged_batch(amount_vars, seg_off, minus_one.repeat(transfers, 1).contiguous(),
                                                  limit.repeat(accounts, 1).contiguous())   # limit - sum of the account's amounts
    composer.range_gate_batch(headroom, 16)                                      # ... is not negative
    n = composer.circuit_size()
    assert composer.check() == -1
    print("%d transfers of %d accounts under their limits: %d rows" % (transfers, accounts, n))

    t = time.perf_counter()
    padded = 1 << (n - 1).bit_length()
    full = composer.materialize()                          # constant columns, fourth wire, wire values
    sigma = composer.permutation(padded)                   # copy permutation, int64[4, padded]
    torch.cuda.synchronize()
    t_ready = time.perf_counter() - t
    print("%d witnesses and the limit check -> %d rows, %d variables: the witnesses' rows built in %.2f ms (%.3g constraints/s), prover-ready in another %.2f ms"
          % (batch, n, composer.num_variables(), t_build * 1e3, built_rows / t_build, t_ready * 1e3))
    assert full["q_arith"].shape == (n, 4) and sigma.shape == (4, padded)
    min_of_two(engine)


def min_of_two(engine, pairs=8):
    """min(x, y) = y + [x <= y] (x - y) of two 64-bit amounts; proven, then verified"""
    S = pg.BlsScalar.from_int
    rnd = np.random.default_rng(7)
    xs = [int(v) for v in rnd.integers(0, 1 << 63, pairs)]
    ys = [int(v) for v in rnd.integers(0, 1 << 63, pairs)]
    ys[0], xs[1] = xs[0], 2**64 - 1                                              # a tie, and the largest amount
    composer = pg.StandardComposer(engine)
    composer.auto_grow()
    first = composer.add_input_batch(torch.from_numpy(synth.scalars_from_ints(xs + ys).view(np.int64)).to("cuda:0"))
    x = torch.arange(first, first + pairs, dtype=torch.int64, device="cuda:0")
    y = x + pairs
    composer.range_gate_batch(x, 64)                                             # the comparison's precondition: both below 2^64
    composer.range_gate_batch(y, 64)
    bit = composer.is_less_equal_each(x, y, 64)                                  # [x <= y], 12 rows an item
    diff = composer.add_batch(S(1), x, S(synth.Q - 1), y, S(0))                  # x - y (in the field)
    part = composer.conditionally_select_zero_batch(diff, bit)                   # x - y where x <= y, else 0
    smaller = composer.add_batch(S(1), y, S(1), part, S(0))
    composer.sync()
    assert composer.check() == -1
    values = np.ascontiguousarray(np.asarray(composer.export()["var_values"])).view(np.uint64).reshape(-1, 4)
    assert [synth.to_int(values[v]) for v in smaller.cpu().tolist()] == [min(a, b) for a, b in zip(xs, ys)]
    n = 1 << (composer.circuit_size() - 1).bit_length()
    tau = S(0x5EED_7A0 ** 9)
    ck, ok = pg.CommitKey.setup(engine, n + 7, tau), pg.OpeningKey.setup(engine, tau)
    pre = composer.preprocessed_commitments(ck)
    proof = composer.prove(ck, b"plonk", pre, blinding=True)
    assert proof.verify(pg.VerifierKey(n, pre), ok, {})
    print("min(x, y) of %d pairs of 64-bit amounts: %d rows, proven (blinded, %d bytes) and verified"
          % (pairs, composer.circuit_size(), len(proof.to_bytes())))
    ok.close()
    composer.close()


if __name__ == "__main__":
    main()
