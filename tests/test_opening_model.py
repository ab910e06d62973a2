"""CPU: the Python-integer model of the opening (tests/opening_model.py) that tests/test_gpu_poly_open.py compares the device
against: (X^2 - 1) / (X - 1) = X + 1, q(y) (y - x) + f(x) = f(y) at random y, x = 0 shifts the coefficients down by one."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import opening_model as M  # noqa: E402


def test_x_squared_minus_one_over_x_minus_one():
    q, rem = M.ruffini([M.R - 1, 0, 1], 1)
    assert q == [1, 1, 0] and rem == 0


def test_division_identity_at_random_points():
    rng = random.Random(12)
    for n in (1, 2, 3, 17, 64):
        f = [rng.randrange(M.R) for _ in range(n)]
        x = rng.randrange(M.R)
        q, rem = M.ruffini(f, x)
        assert q[-1] == 0 and len(q) == n
        assert rem == M.horner(f, x)
        for _ in range(3):
            y = rng.randrange(M.R)
            assert (M.horner(q, y) * (y - x) + rem) % M.R == M.horner(f, y)


def test_zero_point_shifts_down():
    rng = random.Random(3)
    f = [rng.randrange(M.R) for _ in range(9)]
    q, rem = M.ruffini(f, 0)
    assert q == f[1:] + [0] and rem == f[0]


def test_combine_is_linear():
    rng = random.Random(5)
    cols = [[rng.randrange(M.R) for _ in range(7)] for _ in range(3)]
    mu = [1, 0, M.R - 1]
    assert M.combine(cols, mu) == [(a - c) % M.R for a, c in zip(cols[0], cols[2])]
    x = rng.randrange(M.R)
    q, rem = M.open_(cols, mu, x)
    assert rem == sum(m * M.horner(c, x) for m, c in zip(mu, cols)) % M.R
