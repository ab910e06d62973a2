// tests/cpp/sides_device_ops.hip -- test-only harness: the transcript replay of plonk_gadgets_amd/csrc/plonk_sides.hpp
// (sides_challenges<S>, the same header the library includes) started from ANY seed, and fr_from_wide on its own, so that
// tests/test_sides_replay_host.py and tests/test_gpu_sides_replay.py can compare both with Python's Transcript and with big
// integers.  Built by tests/cpp/sides_device_build.py; no inline asm of its own.
//
// The device replay is laid out as plonk_sides_kernel lays it out: workgroups of kSidesLanes = 64 lanes, one proof per lane, the
// sponge of lane l in the words lds[i * 64 + l] of LDS.  A seed whose pos or pos_begin is out of range (what plonk_sides_one
// refuses as a bad key) is not replayed: its seven outputs are all-ones limbs.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../plonk_gadgets_amd/csrc/plonk_sides.hpp"

using pg::Fr;

namespace {

PG_HD bool seed_in_range(uint32_t pos, uint32_t pos_begin) { return pos < pg::kStrobeR && pos_begin <= pg::kStrobeR; }

template <int S>
PG_HD void replay_one(const uint8_t *proof, const uint8_t *state, uint32_t pos, uint32_t pos_begin, uint32_t *mem, Fr *out) {
    Fr ch[pg::kSidesChallenges];
    if (seed_in_range(pos, pos_begin)) {
        for (uint32_t i = 0; i < pg::kSidesStateWords; i++)
            mem[i * S] = (uint32_t)state[4 * i] | (uint32_t)state[4 * i + 1] << 8 | (uint32_t)state[4 * i + 2] << 16 | (uint32_t)state[4 * i + 3] << 24;
        pg::sides_challenges<S>(proof, mem, pos, pos_begin, ch);
    } else {
        for (uint32_t k = 0; k < pg::kSidesChallenges; k++) ch[k] = Fr{{~0ull, ~0ull, ~0ull, ~0ull}};
    }
    for (uint32_t k = 0; k < pg::kSidesChallenges; k++) out[k] = ch[k];
}

__global__ __launch_bounds__(pg::kSidesLanes) void replay_kernel(const uint8_t *proofs, uint64_t n, const uint8_t *states, const uint8_t *pos,
                                                                 const uint8_t *pos_begin, Fr *out) {
    __shared__ uint32_t lds[pg::kSidesWords * pg::kSidesLanes];
    const uint64_t i = (uint64_t)blockIdx.x * pg::kSidesLanes + threadIdx.x;
    if (i >= n) return;
    replay_one<(int)pg::kSidesLanes>(proofs + i * pg::kProofBytes, states + i * 200, pos[i], pos_begin[i], lds + threadIdx.x,
                                     out + i * pg::kSidesChallenges);
}

__global__ void from_wide_kernel(const Fr *lo, const Fr *hi, Fr *out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = pg::fr_from_wide(lo[i], hi[i]);
}

}  // namespace

extern "C" {

// host pointers: proofs n x 1040 bytes, states n x 200, pos / pos_begin n bytes, out n x 7 Fr (Montgomery form)
int sides_replay_host(const uint8_t *proofs, uint64_t n, const uint8_t *states, const uint8_t *pos, const uint8_t *pos_begin, Fr *out) {
    for (uint64_t i = 0; i < n; i++) {
        uint32_t mem[pg::kSidesWords];
        replay_one<1>(proofs + i * pg::kProofBytes, states + i * 200, pos[i], pos_begin[i], mem, out + i * pg::kSidesChallenges);
    }
    return 0;
}

// device pointers, the null stream; block must be kSidesLanes and grid x block must cover n
int sides_replay_device(const uint8_t *proofs, uint64_t n, const uint8_t *states, const uint8_t *pos, const uint8_t *pos_begin, Fr *out,
                        int grid, int block) {
    if (block != (int)pg::kSidesLanes || grid <= 0 || (uint64_t)grid * pg::kSidesLanes < n) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(replay_kernel, dim3((uint32_t)grid), dim3(pg::kSidesLanes), 0, 0, proofs, n, states, pos, pos_begin, out);
    return (int)hipGetLastError();
}

int fr_from_wide_host(const Fr *lo, const Fr *hi, Fr *out, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) out[i] = pg::fr_from_wide(lo[i], hi[i]);
    return 0;
}

int fr_from_wide_device(const Fr *lo, const Fr *hi, Fr *out, uint64_t n, int grid, int block) {
    if (block <= 0 || block > 1024 || grid <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(from_wide_kernel, dim3((uint32_t)grid), dim3((uint32_t)block), 0, 0, lo, hi, out, n);
    return (int)hipGetLastError();
}

}  // extern "C"
