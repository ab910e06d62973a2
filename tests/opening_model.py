"""Python-integer model of round 5's device work (csrc/opening.hpp): the weighted sum of columns and its Ruffini division by
(X - x), coefficients lowest first, over the scalar field."""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def combine(cols, mu):
    """sum_j mu_j p_j, coefficient by coefficient"""
    n = len(cols[0])
    out = [0] * n
    for c, m in zip(cols, mu):
        for i in range(n):
            out[i] = (out[i] + m * c[i]) % R
    return out


def ruffini(f, x):
    """f = q (X - x) + rem -> (q padded to len(f) with a top 0, rem): q_{n-2} = f_{n-1}, q_{i-1} = f_i + x q_i"""
    n = len(f)
    q = [0] * n
    acc = 0
    for i in range(n - 1, 0, -1):
        acc = (f[i] + x * acc) % R
        q[i - 1] = acc
    return q, (f[0] + x * acc) % R


def horner(c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % R
    return acc


def open_(cols, mu, x):
    return ruffini(combine(cols, mu), x)
