"""TEST INFRASTRUCTURE: short random composer programs with weighted_sum_ragged_batch among the other batched appends, made call for
call on the device composer and on the C oracle's (tests/weighted_sum_oracle.Both); dev = None runs the oracle side alone.

Everything comes from the seed.  The program knows of every Variable a public interval [lo, hi] that holds its value, so that a
range widget only takes Variables that fit it and check() is -1 unless a failure is planted.  With probability 1/2 one is, on the
RESULT of a sum (a sum's own rows hold by construction on both sides: both compute the assignments they state): a
constrain_to_constant of the result to a constant outside its interval, or a range gate too narrow for a sum whose constant alone
is beyond it.  Both.planted_row is the row check() must name."""
import random

from tests import weighted_sum_oracle as wso

R = wso.R
STEPS = 15
OPERATIONS = ("add_input_batch", "add_batch", "mul_batch", "interval_gate_ragged_batch", "range_gate_batch", "maybe_equal_batch",
              "range_check_batch") + ("weighted_sum_ragged_batch",) * 4
SMALL = 1 << 200
# chosen against the oracle: tests/test_weighted_sum_model.py asserts what they reach
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)


def even_bits(hi):
    b = max(2, hi.bit_length())
    return b + (b & 1)


def run_program(dev, seed, steps=STEPS):
    rng = random.Random(seed)
    both = wso.Both(dev)
    both.reached, both.planted, both.planted_row = set(), False, None
    known = {both.zero_var: (0, 0)}
    sums = []                      # result Variables of sums
    plant_at = rng.randrange(steps) if rng.random() < 0.5 else None

    def learn(vs, lo, hi):
        for v in vs:
            known[v] = (lo, hi)

    def earlier(k, most=SMALL):
        fit = sorted(v for v, (_, hi) in known.items() if hi < most)
        return [rng.choice(fit) for _ in range(k)]

    def drawn(lo, hi):
        return rng.choice([lo, hi, rng.randrange(lo, hi + 1)])

    def a_sum(constant_floor=0):
        segments = rng.randrange(1, 7)
        sizes = [rng.choice([2, 2, 3, rng.randrange(2, 10)]) for _ in range(segments)]
        off = [0]
        for m in sizes:
            off.append(off[-1] + m)
        x = earlier(off[-1])
        if sums:                   # results of earlier sums among the terms
            for i in rng.sample(range(len(x)), min(len(x), 1 + len(x) // 4)):
                x[i] = rng.choice(sums)
        if any(v in sums for v in x):
            both.reached.add("sum_of_sums")
        co = None if rng.random() < 0.3 else [rng.choice([0, 1, 1, 2, rng.randrange(8)]) for _ in x]
        ks = None if rng.random() < 0.3 and not constant_floor else [constant_floor + rng.choice([0, 1, rng.randrange(1 << 16)]) for _ in sizes]
        res = both.weighted_sum_ragged_batch(x, off, co, ks)
        for s, r in enumerate(res):
            ts = range(off[s], off[s + 1])
            c = [1] * len(x) if co is None else co
            k = 0 if ks is None else ks[s]
            known[r] = (k + sum(c[t] * known[x[t]][0] for t in ts), k + sum(c[t] * known[x[t]][1] for t in ts))
        sums.extend(res)
        return res

    learn(both.add_input_batch([rng.randrange(1 << 16) for _ in range(8)]), 0, (1 << 16) - 1)
    for step in range(steps):
        if step == plant_at:
            both.planted = True
            both.reached.add("failure_on_a_sum_result")
            if rng.random() < 0.5:
                r = rng.choice(a_sum())
                both.planted_row = both.ora.n
                both.constrain_to_constant(r, known[r][1] + 1)
            else:
                res = a_sum(constant_floor=1 << 20)   # every result >= 2^20
                both.planted_row = both.ora.n
                both.range_gate_batch(res, 16)
                both.reached.add("sum_then_range_gate")
            continue
        op = rng.choice(OPERATIONS)
        k = rng.randrange(1, 30)
        if op == "add_input_batch":
            b = rng.choice([8, 16, 32])
            learn(both.add_input_batch([drawn(0, 2**b - 1) for _ in range(k)]), 0, 2**b - 1)
        elif op == "add_batch":
            c = rng.choice([0, 1, rng.randrange(1 << 20)])
            a, b = earlier(k), earlier(k)
            for r, x, y in zip(both.add_batch(1, a, 1, b, c), a, b):
                known[r] = (known[x][0] + known[y][0] + c, known[x][1] + known[y][1] + c)
        elif op == "mul_batch":
            a, b = earlier(k, 1 << 100), earlier(k, 1 << 100)
            for r, x, y in zip(both.mul_batch(1, a, b, 0), a, b):
                known[r] = (known[x][0] * known[y][0], known[x][1] * known[y][1])
        elif op == "maybe_equal_batch":
            learn(both.maybe_equal_batch(earlier(k), earlier(k)), 0, 1)
        elif op == "range_check_batch":
            mx = rng.randrange(2, 1 << rng.randrange(2, 30))
            learn(both.range_check_batch(rng.randrange(0, mx), mx, [drawn(0, 2 * mx) for _ in range(min(k, 4))]), 0, 1)
        elif op == "interval_gate_ragged_batch":
            los = [rng.choice([0, rng.randrange(1 << 30)]) for _ in range(k)]
            his = [lo + rng.randrange(1 << 16) for lo in los]
            ws = both.add_input_batch([drawn(lo, hi) for lo, hi in zip(los, his)])
            for w, lo, hi in zip(ws, los, his):
                known[w] = (lo, hi)
            both.interval_gate_ragged_batch(ws, los, his, 16)
        elif op == "range_gate_batch":
            ws = (rng.sample(sums, min(len(sums), 3)) if sums else []) + earlier(k, 1 << 250)
            ws = [w for w in ws if known[w][1] < (1 << 250)]
            if any(w in sums for w in ws):
                both.reached.add("sum_then_range_gate")
            both.range_gate_batch(ws, even_bits(max(known[w][1] for w in ws)))
        else:
            a_sum()
    return both
