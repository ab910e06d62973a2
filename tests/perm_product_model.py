"""TEST INFRASTRUCTURE: the copy permutation as field elements in plain Python integers mod q -- the statement
pg_sigma_evaluations and pg_permutation_product are compared with, limb for limb.

Conventions [DEP-RECALL] (dusk-plonk 0.8 / dusk-bls12_381, not pinned here: their source is absent):
  k = (1, K1, K2, K3) = (1, 7, 13, 17), one coset constant per wire (left, right, output, fourth: sigma's wire order);
  omega of the 2^m subgroup = ROOT_OF_UNITY^(2^(32 - m)), ROOT_OF_UNITY = 7^t with q - 1 = 2^32 t;
  sigma evaluation of s = sigma[p]:  k[s // padded_n] * omega^(s % padded_n);
  num_i = prod_j (w_j[i] + beta k_j omega^i + gamma), den_i = prod_j (w_j[i] + beta sigma_eval_j[i] + gamma),
  z[0] = 1, z[i] = prod_{r < i} num_r / den_r, wrap = the product of all padded_n ratios; wire values of rows >= n_values are 0."""
import numpy as np

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R = (1 << 256) % Q
RINV = pow(R, -1, Q)
ROOT_OF_UNITY = 0x16A2A19EDFE81F20D09B681922C813B4B63683508C2280B93829971F439F0D2B
K = (1, 7, 13, 17)


def omega_of(m: int) -> int:
    return pow(ROOT_OF_UNITY, 1 << (32 - m), Q)


def from_mont(limbs) -> int:
    return sum(int(x) << (64 * i) for i, x in enumerate(limbs)) * RINV % Q


def mont(x: int) -> list:
    m = x % Q * R % Q
    return [(m >> (64 * i)) & (2**64 - 1) for i in range(4)]


def ints_of(arr) -> list:
    """Montgomery limbs (uint64 / int64 [n, 4]) -> canonical ints"""
    a = np.asarray(arr).view(np.uint64).reshape(-1, 4)
    return [from_mont(r) for r in a.tolist()]


def limbs_of(xs) -> np.ndarray:
    return np.array([mont(x) for x in xs], dtype=np.uint64).reshape(-1, 4)


def powers(omega: int, count: int) -> list:
    out, x = [], 1
    for _ in range(count):
        out.append(x)
        x = x * omega % Q
    return out


def sigma_evaluations(sigma, padded_n: int, omega: int, k=K) -> list:
    """sigma: uint64 [4, padded_n] -> four lists of ints"""
    s = np.asarray(sigma).view(np.uint64).reshape(4, padded_n)
    pw = powers(omega, padded_n)
    return [[k[int(x) // padded_n] * pw[int(x) % padded_n] % Q for x in s[j].tolist()] for j in range(4)]


def factors(wires, sev, i: int, beta: int, gamma: int, omega_i: int, k=K):
    """(num_i, den_i) of row i: wires = four lists of ints (n_values each), sev = the four sigma evaluations of row i"""
    num = den = 1
    for j in range(4):
        w = wires[j][i] if i < len(wires[j]) else 0
        num = num * (w + beta * k[j] * omega_i + gamma) % Q
        den = den * (w + beta * sev[j] + gamma) % Q
    return num, den


def grand_product(wires, sigma, padded_n: int, beta: int, gamma: int, omega: int, k=K):
    """-> (z: list of padded_n ints, wrap)"""
    sev = sigma_evaluations(sigma, padded_n, omega, k)
    z, acc, w_i = [], 1, 1
    for i in range(padded_n):
        z.append(acc)
        num, den = factors(wires, [sev[j][i] for j in range(4)], i, beta, gamma, w_i, k)
        acc = acc * num % Q * pow(den, -1, Q) % Q
        w_i = w_i * omega % Q
    return z, acc
