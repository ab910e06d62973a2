"""Big-integer model of csrc/fr.hpp, limb for limb, and an edge corpus for its device forms (Python ints only).

Values are the integers the four 64-bit limbs store: Montgomery residues a = xR mod q, R = 2^256, every value below q valid.
Besides the plain reference of each operation this models how the gfx950 code computes: `mul_trace` follows fr_mul's
8 x 32-bit product scanning (quotient digit m_k = -lo of each column) and `invert_steps` follows fr_invert_or_zero's division
steps (divsteps_30, zeta form), so that the corpus can be shown to reach the cases uniform inputs almost never reach."""
from __future__ import annotations

import functools
import random

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R = 1 << 256
R_MOD = R % Q
R_INV = pow(R, -1, Q)
M32 = 0xFFFFFFFF
Q_WORDS = [(Q >> (32 * i)) & M32 for i in range(8)]
BATCH_STEPS, BATCHES = 30, 20  # fr_invert_or_zero: 20 batches of 30 division steps


def mont(x: int) -> int:
    return x * R % Q


def words(x: int) -> list[int]:
    return [(x >> (32 * i)) & M32 for i in range(8)]


def from_words(w) -> int:
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


# ---- the operations, on the stored values -----------------------------------------------------------------------
def add(a, b): return (a + b) % Q
def sub(a, b): return (a - b) % Q
def neg(a): return (-a) % Q
def mul(a, b): return a * b * R_INV % Q
def square(a): return mul(a, a)
def to_mont(raw): return raw * R % Q               # fr_to_mont: raw integer -> Montgomery residue
def from_mont(a): return a * R_INV % Q             # fr_from_mont: Montgomery residue -> raw integer
def invert(a): return 0 if a == 0 else R * R * pow(a, Q - 2, Q) % Q  # (xR)^-1 -> x^-1 R; 0 -> 0
def pow_of_2(by): return mont(pow(2, by, Q))
def bits_count(a): return max(1, from_mont(a).bit_length())
def num_bits_closest_power_of_two(a): return bits_count(pow_of_2(bits_count(a)))


def chain(x: int, y: int, steps: int) -> int:
    """the dependent chain the device harness runs per lane: x <- x*y + (x - y)"""
    for _ in range(steps):
        x = add(mul(x, y), sub(x, y))
    return x


# ---- how the device computes -------------------------------------------------------------------------------------
def mul_trace(a: int, b: int) -> dict:
    """fr_mul's gfx950 schedule word by word: per column k < 8 whether the low word was 0 before the quotient digit
    (the `v_cmp_ne_u32` carry), the value before the final subtraction and whether that subtraction was taken"""
    A, B = words(a), words(b)
    m, r, lo_zero = [0] * 8, [0] * 8, []
    acc = 0  # the 96-bit accumulator {ex:hi:lo}
    for k in range(8):
        acc += sum(A[i] * B[k - i] for i in range(k + 1)) + sum(m[i] * Q_WORDS[k - i] for i in range(k))
        lo = acc & M32
        lo_zero.append(lo == 0)
        m[k] = -lo & M32
        acc = (acc + m[k]) >> 32  # m_k * q_0 = m_k zeroes the low word
    for k in range(8, 15):
        acc += sum(A[i] * B[k - i] + m[i] * Q_WORDS[k - i] for i in range(k - 7, 8))
        r[k - 8] = acc & M32
        acc >>= 32
    r[7] = acc & M32
    pre = from_words(r) + ((acc >> 32) << 256)
    assert acc >> 64 == 0 and pre < 2 * Q
    taken = pre >= Q
    return {"lo_zero": lo_zero, "pre": pre, "sub_taken": taken, "value": pre - Q if taken else pre}


def add_sub_taken(a: int, b: int) -> bool:
    return a + b >= Q


def sub_borrow(a: int, b: int) -> bool:
    return a < b


def invert_steps(a: int) -> int:
    """division steps fr_invert_or_zero needs on a (until g = 0): divsteps_30 on whole integers, zeta = -(delta + 1/2)
    starting at -1, (f, g) = (q, a)"""
    f, g, zeta, n = Q, a, -1, 0
    while g:
        if g & 1:
            if zeta < 0:  # delta > 0: swap
                f, g, zeta = g, g - f, -zeta - 2
            else:
                g, zeta = g + f, zeta - 1
        else:
            zeta -= 1
        g >>= 1
        n += 1
    assert a == 0 or abs(f) == 1
    return n


def invert_batches(a: int) -> int:
    """30-step batches a wave holding only `a` runs (the early exit is tested after each batch)"""
    return max(1, -(-invert_steps(a) // BATCH_STEPS))


# ---- the corpus --------------------------------------------------------------------------------------------------
WORD_PATTERNS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)


def named_values() -> list[int]:
    v = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2, R_MOD, R_INV, R * R % Q, mont(1), mont(Q - 1)]
    for k in range(257):
        v += [(1 << k) % Q, ((1 << k) - 1) % Q, (Q - (1 << k)) % Q]
    return v


def word_pattern_values(n: int, rng: random.Random) -> list[int]:
    out = [from_words([p] * 8) for p in WORD_PATTERNS]
    while len(out) < n:
        out.append(from_words([rng.choice(WORD_PATTERNS + (Q_WORDS[i],)) for i in range(8)]))
    return [x for x in out if x < Q]


def column_pairs(rng: random.Random, per_target: int = 2) -> list[tuple[int, int]]:
    """per column k, pairs whose low word before the quotient digit is 0, 1 or 0xffffffff: with every other word of b
    fixed the low word of column k is S + a_0 b_k (mod 2^32), so b_k = (t - S) a_0^-1"""
    out = []
    for k in range(8):
        for t in (0, 1, M32):
            got = 0
            while got < per_target:
                a = rng.randrange(Q) | 1  # a_0 odd: invertible mod 2^32
                bw = [rng.getrandbits(32) for _ in range(7)] + [rng.randrange(Q_WORDS[7])]
                bw[k] = 0
                s = _column_lo(a, from_words(bw), k)
                bw[k] = (t - s) * pow(a & M32, -1, 1 << 32) & M32
                b = from_words(bw)
                if a >= Q or b >= Q:
                    continue
                assert _column_lo(a, b, k) == t
                out.append((a, b))
                got += 1
    return out


def _column_lo(a: int, b: int, k: int) -> int:
    A, B = words(a), words(b)
    m, acc = [0] * 8, 0
    for j in range(k + 1):
        acc += sum(A[i] * B[j - i] for i in range(j + 1)) + sum(m[i] * Q_WORDS[j - i] for i in range(j))
        lo = acc & M32
        if j == k:
            return lo
        m[j] = -lo & M32
        acc = (acc + m[j]) >> 32


def final_sub_pairs(rng: random.Random, per_kind: int = 8) -> list[tuple[int, int]]:
    """products whose value before the final subtraction lies just above q (result c near 0) or just below it (result
    c near q - 1): fix b and c, solve a = c R b^-1, keep the pairs that land on the wanted side"""
    above, below = [], []
    while len(above) < per_kind or len(below) < per_kind:
        b = rng.randrange(1, Q)
        c = rng.randrange(4) if len(above) < per_kind else Q - 1 - rng.randrange(4)
        a = c * R * pow(b, -1, Q) % Q
        t = mul_trace(a, b)
        if c < 4 and t["sub_taken"] and len(above) < per_kind:
            above.append((a, b))
        elif c >= Q - 4 and not t["sub_taken"] and len(below) < per_kind:
            below.append((a, b))
    return above + below


def add_sub_pairs(rng: random.Random) -> list[tuple[int, int]]:
    out = [(0, Q - 1), (Q - 1, 0), (Q - 1, Q - 1), (0, 0)]
    for _ in range(16):
        a = rng.randrange(Q)
        for s in (Q - 1, Q, Q + 1, 2 * Q - 2):  # a + b
            if 0 <= s - a < Q:
                out.append((a, s - a))
        for d in (-1, 0, 1):  # a - b
            if 0 <= a - d < Q:
                out.append((a, a - d))
    return out


@functools.lru_cache(maxsize=None)
def corpus(seed: int = 2024) -> dict[str, list[tuple[int, int]]]:
    """the edge corpus by class: pairs (a, b) of values below q; one-operand operations take both members"""
    rng = random.Random(seed)
    named = named_values()
    pats = word_pattern_values(1024, rng)
    return {
        "named": [(a, b) for a, b in zip(named, named[1:] + named[:1])] + [(x, x) for x in named[:12]],
        "named_cross": [(a, b) for a in named[:12] for b in named[:12]],
        "word_patterns": list(zip(pats, pats[1:] + pats[:1])),
        "mul_columns": column_pairs(rng),
        "mul_final_sub": final_sub_pairs(rng),
        "add_sub_boundaries": add_sub_pairs(rng),
    }


def corpus_pairs(seed: int = 2024) -> list[tuple[int, int]]:
    return [p for ps in corpus(seed).values() for p in ps]


@functools.lru_cache(maxsize=None)
def corpus_values(seed: int = 2024) -> list[int]:
    return tuple(sorted({x for p in corpus_pairs(seed) for x in p}))


def slow_inversion_inputs(min_batches: int = 17) -> list[int]:
    """the named values whose inversion needs at least `min_batches` batches (the 2^k - 1 and q - 2^k families)"""
    return [x for x in dict.fromkeys(named_values()) if invert_batches(x) >= min_batches]
