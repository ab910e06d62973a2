// tests/cpp/fr_device_ops.hip -- test-only harness: the library's field arithmetic (plonk_gadgets_amd/csrc/fr.hpp, the same
// header the kernels include) one operation at a time, so that tests/test_gpu_fr_device.py can compare every device form
// with a big-integer model limb for limb.  Built by tests/cpp/fr_device_build.py; no inline asm of its own.
//
// Every launcher takes device pointers and the launch shape (block size, grid), runs a grid-stride loop over n elements
// on the null stream and returns the HIP status of the launch.  A test picks the shape: full occupancy, one wave per
// workgroup (a wave alone on its SIMD, issuing back to back), or an n that leaves the last wave partial.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../plonk_gadgets_amd/csrc/fr.hpp"

using pg::Fr;

namespace {

enum Unary { NEG = 0, SQUARE, TO_MONT, FROM_MONT, INVERT_OR_ZERO, INVERT_FERMAT };
enum Binary { ADD = 0, SUB, MUL };

#define FR_GRID_LOOP(i) for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)

template <int OP>
__global__ void unary_kernel(const Fr *a, Fr *out, uint64_t n) {
    FR_GRID_LOOP(i) {
        const Fr x = a[i];
        Fr r;
        if constexpr (OP == NEG) r = pg::fr_neg(x);
        else if constexpr (OP == SQUARE) r = pg::fr_square(x);
        else if constexpr (OP == TO_MONT) r = pg::fr_to_mont(x);
        else if constexpr (OP == FROM_MONT) r = pg::fr_from_mont(x);
        else if constexpr (OP == INVERT_OR_ZERO) r = pg::fr_invert_or_zero(x);
        else r = pg::fr_invert_fermat(x);
        out[i] = r;
    }
}

template <int OP>
__global__ void binary_kernel(const Fr *a, const Fr *b, Fr *out, uint64_t n) {
    FR_GRID_LOOP(i) {
        const Fr x = a[i], y = b[i];
        if constexpr (OP == ADD) out[i] = pg::fr_add(x, y);
        else if constexpr (OP == SUB) out[i] = pg::fr_sub(x, y);
        else out[i] = pg::fr_mul(x, y);
    }
}

__global__ void pow_of_2_kernel(const uint64_t *by, Fr *out, uint64_t n) {
    FR_GRID_LOOP(i) out[i] = pg::fr_pow_of_2(by[i]);
}

__global__ void bits_kernel(const Fr *a, uint64_t *count, uint64_t *closest, uint64_t n) {
    FR_GRID_LOOP(i) {
        count[i] = pg::bits_count(a[i]);
        closest[i] = pg::num_bits_closest_power_of_two(a[i]);
    }
}

// x <- x*y + (x - y), `steps` times: one wrong carry anywhere shows in the final value
PG_HD Fr chain_step(const Fr &x, const Fr &y) { return pg::fr_add(pg::fr_mul(x, y), pg::fr_sub(x, y)); }

__global__ void chain_kernel(const Fr *x0, const Fr *y, Fr *out, uint64_t n, uint32_t steps) {
    FR_GRID_LOOP(i) {
        Fr x = x0[i];
        const Fr yy = y[i];
        for (uint32_t s = 0; s < steps; s++) x = chain_step(x, yy);
        out[i] = x;
    }
}

// the inversion inside a lane-divergent branch (invert.hpp: `if (any) accinv = fr_invert_or_zero(acc)`): inactive lanes
// keep their input
__global__ void masked_invert_kernel(const Fr *a, const uint8_t *active, Fr *out, uint64_t n) {
    FR_GRID_LOOP(i) {
        Fr r = a[i];
        if (active[i]) r = pg::fr_invert_or_zero(r);
        out[i] = r;
    }
}

template <typename K, typename... Args>
int launch(K kernel, int block, int grid, Args... args) {
    if (block <= 0 || block > 1024 || grid <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3((uint32_t)block), 0, 0, args...);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// op: 0 neg, 1 square, 2 to_mont, 3 from_mont, 4 invert_or_zero, 5 invert_fermat
int fr_dev_unary(int op, const Fr *a, Fr *out, uint64_t n, int block, int grid) {
    switch (op) {
        case NEG: return launch(unary_kernel<NEG>, block, grid, a, out, n);
        case SQUARE: return launch(unary_kernel<SQUARE>, block, grid, a, out, n);
        case TO_MONT: return launch(unary_kernel<TO_MONT>, block, grid, a, out, n);
        case FROM_MONT: return launch(unary_kernel<FROM_MONT>, block, grid, a, out, n);
        case INVERT_OR_ZERO: return launch(unary_kernel<INVERT_OR_ZERO>, block, grid, a, out, n);
        case INVERT_FERMAT: return launch(unary_kernel<INVERT_FERMAT>, block, grid, a, out, n);
        default: return (int)hipErrorInvalidValue;
    }
}

// op: 0 add, 1 sub, 2 mul
int fr_dev_binary(int op, const Fr *a, const Fr *b, Fr *out, uint64_t n, int block, int grid) {
    switch (op) {
        case ADD: return launch(binary_kernel<ADD>, block, grid, a, b, out, n);
        case SUB: return launch(binary_kernel<SUB>, block, grid, a, b, out, n);
        case MUL: return launch(binary_kernel<MUL>, block, grid, a, b, out, n);
        default: return (int)hipErrorInvalidValue;
    }
}

int fr_dev_pow_of_2(const uint64_t *by, Fr *out, uint64_t n, int block, int grid) {
    return launch(pow_of_2_kernel, block, grid, by, out, n);
}

int fr_dev_bits(const Fr *a, uint64_t *count, uint64_t *closest, uint64_t n, int block, int grid) {
    return launch(bits_kernel, block, grid, a, count, closest, n);
}

int fr_dev_chain(const Fr *x, const Fr *y, Fr *out, uint64_t n, uint32_t steps, int block, int grid) {
    return launch(chain_kernel, block, grid, x, y, out, n, steps);
}

int fr_dev_masked_invert(const Fr *a, const uint8_t *active, Fr *out, uint64_t n, int block, int grid) {
    return launch(masked_invert_kernel, block, grid, a, active, out, n);
}

// the same chain on the host (host pointers), from the generic forms of fr.hpp; at most 16 threads
int fr_host_chain(const Fr *x, const Fr *y, Fr *out, uint64_t n, uint32_t steps, int threads) {
    const int t = std::max(1, std::min(threads, 16));
    std::vector<std::thread> pool;
    for (int w = 0; w < t; w++)
        pool.emplace_back([=] {
            for (uint64_t i = (uint64_t)w; i < n; i += (uint64_t)t) {
                Fr v = x[i];
                for (uint32_t s = 0; s < steps; s++) v = chain_step(v, y[i]);
                out[i] = v;
            }
        });
    for (auto &th : pool) th.join();
    return 0;
}

}  // extern "C"
