"""TEST INFRASTRUCTURE: NTTs over the scalar field in plain Python integers mod q -- the statement pg_ntt (csrc/ntt.hpp) is compared
with, limb for limb.  dusk-plonk 0.8's EvaluationDomain [DEP-RECALL] on n = 2^m points with omega = perm_product_model.omega_of(m):
  fft(c)[j] = sum_i c_i omega^(ij)            ifft(e)[i] = n^-1 sum_j e_j omega^(-ij)
  coset_fft(c) = fft(c_i g^i)                 coset_ifft(e)[i] = g^-i ifft(e)[i]
Two independent forms: a naive O(n^2) DFT (n <= 2^8) and a recursive radix-2 transform (n <= 2^16)."""
from perm_product_model import Q, omega_of  # noqa: F401

DEFAULT_G = 7  # [DEP-RECALL] dusk-bls12_381's GENERATOR


def dft(c, omega: int) -> list:
    """naive: e_j = sum_i c_i omega^(ij)"""
    n = len(c)
    assert n <= 1 << 8
    out = []
    for j in range(n):
        wj, acc, x = pow(omega, j, Q), 0, 1
        for ci in c:
            acc = (acc + ci * x) % Q
            x = x * wj % Q
        out.append(acc)
    return out


def ntt(c, omega: int) -> list:
    """recursive radix-2 (even / odd split): the same map as dft"""
    n = len(c)
    assert n & (n - 1) == 0 and n <= 1 << 16
    if n == 1:
        return [c[0] % Q]
    w2 = omega * omega % Q
    ev, od = ntt(c[0::2], w2), ntt(c[1::2], w2)
    out, x = [0] * n, 1
    for j in range(n // 2):
        t = x * od[j] % Q
        out[j] = (ev[j] + t) % Q
        out[j + n // 2] = (ev[j] - t) % Q
        x = x * omega % Q
    return out


def _transform(c, omega):
    return dft(c, omega) if len(c) <= 1 << 8 else ntt(c, omega)


def fft(c, omega: int | None = None) -> list:
    return _transform(list(c), omega_of(len(c).bit_length() - 1) if omega is None else omega)


def ifft(e, omega: int | None = None) -> list:
    n = len(e)
    omega = omega_of(n.bit_length() - 1) if omega is None else omega
    n_inv = pow(n, -1, Q)
    return [x * n_inv % Q for x in _transform(list(e), pow(omega, -1, Q))]


def coset_fft(c, g: int = DEFAULT_G, omega: int | None = None) -> list:
    x, s = 1, []
    for ci in c:
        s.append(ci * x % Q)
        x = x * g % Q
    return fft(s, omega)


def coset_ifft(e, g: int = DEFAULT_G, omega: int | None = None) -> list:
    g_inv, x, out = pow(g, -1, Q), 1, []
    for ci in ifft(e, omega):
        out.append(ci * x % Q)
        x = x * g_inv % Q
    return out


KINDS = {"fft": fft, "ifft": ifft, "coset_fft": coset_fft, "coset_ifft": coset_ifft}


def horner(c, x: int) -> int:
    acc = 0
    for ci in reversed(c):
        acc = (acc * x + ci) % Q
    return acc


def point_identity_holds(c, e, s: int, omega: int) -> bool:
    """e = fft(c) on the 2^m subgroup, checked at a random point s (not in the subgroup):
    sum_j e_j s^j == (s^n - 1) sum_i c_i / (omega^i s - 1)  (both sides are sum_i c_i sum_j (omega^i s)^j)"""
    n = len(c)
    lhs = horner(e, s)
    dens, x = [], 1
    for _ in range(n):
        dens.append((x * s - 1) % Q)
        x = x * omega % Q
    # one inversion for all denominators (Montgomery's trick)
    pre, acc = [], 1
    for d in dens:
        pre.append(acc)
        acc = acc * d % Q
    inv = pow(acc, -1, Q)
    rhs = 0
    for i in range(n - 1, -1, -1):
        rhs = (rhs + c[i] * (inv * pre[i] % Q)) % Q
        inv = inv * dens[i] % Q
    return lhs == (pow(s, n, Q) - 1) * rhs % Q


def _point_check_lib(out_dir: str):
    """tests/cpp/ntt_point_check.c with oracle/fr.c as a second source, as a ctypes library"""
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(out_dir, "libntt_point_check.so")
    if not os.path.exists(so):
        subprocess.check_call(["gcc", "-std=c11", "-O2", "-Wall", "-shared", "-fPIC", "-pthread", "-I", os.path.join(root, "oracle"),
                               os.path.join(root, "tests", "cpp", "ntt_point_check.c"), os.path.join(root, "oracle", "fr.c"), "-o", so])
    return C.CDLL(so)


def build_point_check(out_dir: str):
    """ctypes function ntt_point_check(c, e, n, s, omega, threads): the identity above on Montgomery-limb arrays
    (uint64 [n, 4]); 1 holds, 0 fails, -1 s lies in the subgroup"""
    import ctypes as C
    fn = _point_check_lib(out_dir).ntt_point_check
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]
    return fn


def build_point_check_scaled(out_dir: str):
    """ctypes function ntt_point_check_scaled(c, e, n, s, omega, g, threads): the same identity with c_i g^i for c_i, that is
    e = coset_fft(c, g).  One check for all four kinds: fft (c = in, e = out, g = 1), ifft (c = out, e = in, g = 1), coset_fft
    (c = in, e = out, g), coset_ifft (c = out, e = in, g)"""
    import ctypes as C
    fn = _point_check_lib(out_dir).ntt_point_check_scaled
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return fn


def point_check_threads() -> int:
    import os
    try:
        return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))
    except ValueError:
        return 16
