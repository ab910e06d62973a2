// tests/cpp/fq12_device_ops.hip -- test-only harness: the device forms of the pairing's field tower (plonk_gadgets_amd/csrc/fq2.hpp,
// fq12.hpp, the headers pairing.hpp's kernel includes) one operation at a time, so that tests/test_gpu_fq12_device.py can compare
// them with tests/pairing_model.py limb for limb.  Built by tests/cpp/fq12_device_build.py.  Every launcher takes the launch
// shape (blocks, threads per block), runs a grid-stride loop on the null stream and returns the HIP status of the launch.
//   fq2_op:   one lane per element.
//   fq12_op:  one lane per COEFFICIENT, lane i computing coefficient i % 6 of element i / 6 from operands in memory -- the unit of
//             work of pairing_check_kernel's lanes.  Fq12 elements are Fq2[6].
//   fq12_inv: one lane per element (fq12_inverse is single-threaded), 12 Fq2 of workspace per element.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../plonk_gadgets_amd/csrc/fq12.hpp"

using pg::Fq;
using pg::Fq2;

namespace {

enum Op2 { F2_ADD = 0, F2_SUB, F2_NEG, F2_MUL, F2_SQUARE, F2_INVERSE, F2_CONJ, F2_MUL_XI, F2_DBL, F2_MUL_FQ };
enum Op12 { F12_ADD = 0, F12_SUB, F12_NEG, F12_MUL, F12_SQUARE, F12_CONJ, F12_FROB, F12_FROB2, F12_SPARSE };

#define GRID_LOOP(i, n) for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)

template <int OP>
__global__ void fq2_kernel(const Fq2 *a, const Fq2 *b, Fq2 *out, uint64_t n) {
    GRID_LOOP(i, n) {
        const Fq2 x = a[i], y = b[i];
        if constexpr (OP == F2_ADD) out[i] = pg::fq2_add(x, y);
        else if constexpr (OP == F2_SUB) out[i] = pg::fq2_sub(x, y);
        else if constexpr (OP == F2_NEG) out[i] = pg::fq2_neg(x);
        else if constexpr (OP == F2_MUL) out[i] = pg::fq2_mul(x, y);
        else if constexpr (OP == F2_SQUARE) out[i] = pg::fq2_square(x);
        else if constexpr (OP == F2_INVERSE) out[i] = pg::fq2_inverse(x);
        else if constexpr (OP == F2_CONJ) out[i] = pg::fq2_conj(x);
        else if constexpr (OP == F2_MUL_XI) out[i] = pg::fq2_mul_xi(x);
        else if constexpr (OP == F2_DBL) out[i] = pg::fq2_dbl(x);
        else out[i] = pg::fq2_mul_fq(x, y.c0);
    }
}

// lines: per element l0, l2 (Fq2) and l3 (an Fq2 whose c0 is used), 3 Fq2
template <int OP>
__global__ void fq12_kernel(const Fq2 *a, const Fq2 *b, const Fq2 *lines, Fq2 *out, uint64_t n) {
    GRID_LOOP(i, 6 * n) {
        const uint64_t e = i / 6;
        const int k = (int)(i % 6);
        const Fq2 *x = a + 6 * e, *y = b + 6 * e;
        Fq2 r;
        if constexpr (OP == F12_ADD) r = pg::fq2_add(x[k], y[k]);
        else if constexpr (OP == F12_SUB) r = pg::fq2_sub(x[k], y[k]);
        else if constexpr (OP == F12_NEG) r = pg::fq2_neg(x[k]);
        else if constexpr (OP == F12_MUL) r = pg::fq12_mul_coeff(x, y, k);
        else if constexpr (OP == F12_SQUARE) r = pg::fq12_mul_coeff(x, x, k);
        else if constexpr (OP == F12_CONJ) r = pg::fq12_conj_coeff(x[k], k);
        else if constexpr (OP == F12_FROB) r = pg::fq12_frobenius_coeff(x[k], k);
        else if constexpr (OP == F12_FROB2) r = pg::fq12_frobenius2_coeff(x[k], k);
        else r = pg::fq12_sparse_coeff(x, lines[3 * e], lines[3 * e + 1], lines[3 * e + 2].c0, k);
        out[i] = r;
    }
}

__global__ void fq12_inverse_kernel(const Fq2 *a, Fq2 *out, Fq2 *tmp, uint64_t n) {
    GRID_LOOP(i, n) pg::fq12_inverse(a + 6 * i, out + 6 * i, tmp + 12 * i);
}

}  // namespace

extern "C" {

int fq2_op(int op, const void *a, const void *b, void *out, uint64_t n, uint32_t blocks, uint32_t threads) {
    const Fq2 *x = static_cast<const Fq2 *>(a), *y = static_cast<const Fq2 *>(b);
    Fq2 *o = static_cast<Fq2 *>(out);
    if (!blocks || !threads || threads > 1024) return -1;
#define CASE2(OP) case OP: hipLaunchKernelGGL(fq2_kernel<OP>, dim3(blocks), dim3(threads), 0, nullptr, x, y, o, n); break;
    switch (op) {
        CASE2(F2_ADD) CASE2(F2_SUB) CASE2(F2_NEG) CASE2(F2_MUL) CASE2(F2_SQUARE) CASE2(F2_INVERSE) CASE2(F2_CONJ) CASE2(F2_MUL_XI)
        CASE2(F2_DBL) CASE2(F2_MUL_FQ)
        default: return -1;
    }
    return (int)hipGetLastError();
}

int fq12_op(int op, const void *a, const void *b, const void *lines, void *out, uint64_t n, uint32_t blocks, uint32_t threads) {
    const Fq2 *x = static_cast<const Fq2 *>(a), *y = static_cast<const Fq2 *>(b), *l = static_cast<const Fq2 *>(lines);
    Fq2 *o = static_cast<Fq2 *>(out);
    if (!blocks || !threads || threads > 1024) return -1;
#define CASE12(OP) case OP: hipLaunchKernelGGL(fq12_kernel<OP>, dim3(blocks), dim3(threads), 0, nullptr, x, y, l, o, n); break;
    switch (op) {
        CASE12(F12_ADD) CASE12(F12_SUB) CASE12(F12_NEG) CASE12(F12_MUL) CASE12(F12_SQUARE) CASE12(F12_CONJ) CASE12(F12_FROB)
        CASE12(F12_FROB2) CASE12(F12_SPARSE)
        default: return -1;
    }
    return (int)hipGetLastError();
}

int fq12_inv(const void *a, void *out, void *tmp, uint64_t n, uint32_t blocks, uint32_t threads) {
    if (!blocks || !threads || threads > 1024) return -1;
    hipLaunchKernelGGL(fq12_inverse_kernel, dim3(blocks), dim3(threads), 0, nullptr, static_cast<const Fq2 *>(a), static_cast<Fq2 *>(out),
                       static_cast<Fq2 *>(tmp), n);
    return (int)hipGetLastError();
}

}  // extern "C"
