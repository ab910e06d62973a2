// tools/fq_mul_bench.hip -- micro-benchmark of the base-field Montgomery multiplication on gfx950 (the fq_mul ceiling that
// tools/msm_rate.py divides by).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/fq_mul_bench tools/fq_mul_bench.hip && ./tools/fq_mul_bench
// variant 0 = generic 6 x 64-bit code (fq_mul64), variant 1 = the gfx950 form (fq_mul on the device)
// Prints multiplications/s per variant and checks that the variants agree (and a few lanes against the host code).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../plonk_gadgets_amd/csrc/fq.hpp"

using namespace pg;

template <int VARIANT>
__global__ __launch_bounds__(256) void chain_kernel(const Fq *in, Fq *out, int iters) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fq a = in[2 * i], b = in[2 * i + 1];
    for (int k = 0; k < iters; k++) {
        if constexpr (VARIANT == 0) { a = fq_mul64(a, b); b = fq_mul64(b, a); }
        else { a = fq_mul(a, b); b = fq_mul(b, a); }
    }
    out[i] = fq_add(a, b);
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main(int argc, char **argv) {
    const int blocks = argc > 1 ? atoi(argv[1]) : 256 * 8, threads = argc > 2 ? atoi(argv[2]) : 256, iters = 1000;
    const size_t n = (size_t)blocks * threads;
    std::vector<Fq> h(2 * n);
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for (auto &f : h) {
        for (int k = 0; k < 6; k++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; f.l[k] = s; }
        f.l[5] %= PG_P5;
    }
    Fq *d_in, *d_out0, *d_out1;
    CK(hipMalloc(&d_in, 2 * n * sizeof(Fq)));
    CK(hipMalloc(&d_out0, n * sizeof(Fq)));
    CK(hipMalloc(&d_out1, n * sizeof(Fq)));
    CK(hipMemcpy(d_in, h.data(), 2 * n * sizeof(Fq), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int variant = 0; variant < 2; variant++) {
        for (int rep = 0; rep < 2; rep++) {
            CK(hipEventRecord(e0));
            if (variant == 0) hipLaunchKernelGGL(chain_kernel<0>, dim3(blocks), dim3(threads), 0, 0, d_in, d_out0, iters);
            else hipLaunchKernelGGL(chain_kernel<1>, dim3(blocks), dim3(threads), 0, 0, d_in, d_out1, iters);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep) printf("variant %d (%d blocks x %d): %.3f ms, %.3e fq-mul/s\n", variant, blocks, threads, ms, 2.0 * iters * n / (ms * 1e-3));
        }
    }
    std::vector<Fq> o0(n), o1(n);
    CK(hipMemcpy(o0.data(), d_out0, n * sizeof(Fq), hipMemcpyDeviceToHost));
    CK(hipMemcpy(o1.data(), d_out1, n * sizeof(Fq), hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 6; k++) bad += o0[i].l[k] != o1[i].l[k];
    size_t hbad = 0;
    for (size_t i = 0; i < 16; i++) {
        Fq a = h[2 * i], b = h[2 * i + 1];
        for (int k = 0; k < iters; k++) { a = fq_mul64(a, b); b = fq_mul64(b, a); }
        Fq r = fq_add(a, b);
        for (int k = 0; k < 6; k++) hbad += r.l[k] != o1[i].l[k];
    }
    printf("mismatching limbs between variants: %zu; vs host: %zu\n", bad, hbad);
    return bad || hbad ? 2 : 0;
}
