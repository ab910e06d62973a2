// tests/cpp/fq_device_ops.hip -- test-only harness: the base field's device forms (plonk_gadgets_amd/csrc/fq.hpp, the header the
// G1 kernels include) one operation at a time, so that tests/test_gpu_fq_device.py can compare them with a big-integer model
// limb for limb.  Built by tests/cpp/fq_device_build.py.  Every launcher runs a grid-stride loop over n elements on the null
// stream and returns the HIP status of the launch.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../plonk_gadgets_amd/csrc/fq.hpp"

using pg::Fq;

namespace {

enum Unary { NEG = 0, SQUARE, TO_MONT, FROM_MONT, INVERT };
enum Binary { ADD = 0, SUB, MUL };

#define FQ_GRID_LOOP(i) for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)

template <int OP>
__global__ void unary_kernel(const Fq *a, Fq *out, uint64_t n) {
    FQ_GRID_LOOP(i) {
        const Fq x = a[i];
        if constexpr (OP == NEG) out[i] = pg::fq_neg(x);
        else if constexpr (OP == SQUARE) out[i] = pg::fq_square(x);
        else if constexpr (OP == TO_MONT) out[i] = pg::fq_to_mont(x);
        else if constexpr (OP == FROM_MONT) out[i] = pg::fq_from_mont(x);
        else out[i] = pg::fq_invert(x);
    }
}

template <int OP>
__global__ void binary_kernel(const Fq *a, const Fq *b, Fq *out, uint64_t n) {
    FQ_GRID_LOOP(i) {
        const Fq x = a[i], y = b[i];
        if constexpr (OP == ADD) out[i] = pg::fq_add(x, y);
        else if constexpr (OP == SUB) out[i] = pg::fq_sub(x, y);
        else out[i] = pg::fq_mul(x, y);
    }
}

dim3 grid(uint64_t n) { return dim3((uint32_t)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)); }

}  // namespace

extern "C" {

int fq_unary(int op, const void *a, void *out, uint64_t n) {
    const Fq *x = static_cast<const Fq *>(a);
    Fq *o = static_cast<Fq *>(out);
    switch (op) {
        case NEG: hipLaunchKernelGGL(unary_kernel<NEG>, grid(n), dim3(256), 0, nullptr, x, o, n); break;
        case SQUARE: hipLaunchKernelGGL(unary_kernel<SQUARE>, grid(n), dim3(256), 0, nullptr, x, o, n); break;
        case TO_MONT: hipLaunchKernelGGL(unary_kernel<TO_MONT>, grid(n), dim3(256), 0, nullptr, x, o, n); break;
        case FROM_MONT: hipLaunchKernelGGL(unary_kernel<FROM_MONT>, grid(n), dim3(256), 0, nullptr, x, o, n); break;
        case INVERT: hipLaunchKernelGGL(unary_kernel<INVERT>, grid(n), dim3(256), 0, nullptr, x, o, n); break;
        default: return -1;
    }
    return (int)hipGetLastError();
}

int fq_binary(int op, const void *a, const void *b, void *out, uint64_t n) {
    const Fq *x = static_cast<const Fq *>(a), *y = static_cast<const Fq *>(b);
    Fq *o = static_cast<Fq *>(out);
    switch (op) {
        case ADD: hipLaunchKernelGGL(binary_kernel<ADD>, grid(n), dim3(256), 0, nullptr, x, y, o, n); break;
        case SUB: hipLaunchKernelGGL(binary_kernel<SUB>, grid(n), dim3(256), 0, nullptr, x, y, o, n); break;
        case MUL: hipLaunchKernelGGL(binary_kernel<MUL>, grid(n), dim3(256), 0, nullptr, x, y, o, n); break;
        default: return -1;
    }
    return (int)hipGetLastError();
}

}  // extern "C"
