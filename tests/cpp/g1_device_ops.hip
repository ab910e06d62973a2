// tests/cpp/g1_device_ops.hip -- test-only harness: the device forms of the G1 group law (plonk_gadgets_amd/csrc/g1.hpp) one
// operation at a time, and g1_normalize_kernel (csrc/msm.hpp) launched on its own with any batch size, so that
// tests/test_gpu_g1_device.py can compare them with tests/g1_model.py.  Built by tests/cpp/g1_device_build.py.  Every launcher
// runs on the null stream and returns the HIP status of the launch.
//   g1_op:        one lane per element in a grid-stride loop over the launch shape (blocks, threads per block).  a and b hold
//                 G1X (24 limbs) or G1A (12 limbs) rows as the operation says, k one uint32 per element; out holds G1X rows,
//                 G1A rows for NEG_AFFINE.
//   g1_normalize: pg::g1_normalize_kernel over m points with per_lane points per inversion, on the grid capi uses.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>  // (rocPRIM's headers call memset on the host without naming its header)

#include "../../plonk_gadgets_amd/csrc/msm.hpp"

using pg::G1A;
using pg::G1X;

namespace {

enum Op { ADD = 0, ADD_AFFINE, DBL, DBL_AFFINE, MUL_SMALL, FROM_AFFINE, NEG_AFFINE };

#define GRID_LOOP(i, n) for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)

template <int OP>
__global__ void g1_kernel(const void *a, const void *b, const uint32_t *k, void *out, uint64_t n) {
    const G1X *ax = static_cast<const G1X *>(a), *bx = static_cast<const G1X *>(b);
    const G1A *aa = static_cast<const G1A *>(a), *ba = static_cast<const G1A *>(b);
    G1X *ox = static_cast<G1X *>(out);
    GRID_LOOP(i, n) {
        if constexpr (OP == ADD) ox[i] = pg::g1x_add(ax[i], bx[i]);
        else if constexpr (OP == ADD_AFFINE) ox[i] = pg::g1x_add_affine(ax[i], ba[i]);
        else if constexpr (OP == DBL) ox[i] = pg::g1x_dbl(ax[i]);
        else if constexpr (OP == DBL_AFFINE) ox[i] = pg::g1x_dbl_affine(aa[i]);
        else if constexpr (OP == MUL_SMALL) ox[i] = pg::g1x_mul_small(ax[i], k[i]);
        else if constexpr (OP == FROM_AFFINE) ox[i] = pg::g1x_from_affine(aa[i]);
        else static_cast<G1A *>(out)[i] = pg::g1a_neg(aa[i]);
    }
}

}  // namespace

extern "C" {

int g1_op(int op, const void *a, const void *b, const void *k, void *out, uint64_t n, uint32_t blocks, uint32_t threads) {
    const uint32_t *kk = static_cast<const uint32_t *>(k);
    if (!blocks || !threads || threads > 1024) return -1;
#define CASE1(OP) case OP: hipLaunchKernelGGL(g1_kernel<OP>, dim3(blocks), dim3(threads), 0, nullptr, a, b, kk, out, n); break;
    switch (op) {
        CASE1(ADD) CASE1(ADD_AFFINE) CASE1(DBL) CASE1(DBL_AFFINE) CASE1(MUL_SMALL) CASE1(FROM_AFFINE) CASE1(NEG_AFFINE)
        default: return -1;
    }
    return (int)hipGetLastError();
}

int g1_normalize(const void *in, void *out, uint64_t m, uint32_t per_lane) {
    if (!m || !per_lane) return -1;
    const uint64_t lanes = (m + per_lane - 1) / per_lane, blocks = (lanes + pg::kThreads - 1) / pg::kThreads;
    if (blocks >= (1ull << 31)) return -1;
    hipLaunchKernelGGL(pg::g1_normalize_kernel, dim3((uint32_t)blocks), dim3(pg::kThreads), 0, nullptr, static_cast<const G1X *>(in),
                       static_cast<G1A *>(out), m, per_lane);
    return (int)hipGetLastError();
}

}  // extern "C"
