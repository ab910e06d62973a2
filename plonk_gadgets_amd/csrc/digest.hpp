// digest.hpp -- what the preflight of an append on device arrays computes and brings back: the 128-bit digest of the arrays its rows
// depend on (the append is signed with it, pg_composer_clear_witness) and the block of result words the host reads in one copy.
// Compiled by hipcc for the kernels and the composer, and by a plain C++ compiler for tests/cpp/digest_host.cpp.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PG_DIGEST_HD __host__ __device__ __forceinline__
#else
#define PG_DIGEST_HD inline
#endif

namespace pg {

PG_DIGEST_HD unsigned long long digest_mix(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// Sums of two position-salted 64-bit mixes over the words of a call's arrays: the order of summation does not matter (any lane may
// add any word, and partial sums add up), the order of the entries does (`at`: the word's place in its array), and so does the array
// a word stands in (`salt`: one per array of a call, below).
struct Digest {
    unsigned long long h1, h2;
    PG_DIGEST_HD void add(unsigned long long w, unsigned long long at, unsigned long long salt) {
        h1 += digest_mix(w + digest_mix(at + salt));
        h2 += digest_mix((w ^ 0x9e3779b97f4a7c15ull) * 0xff51afd7ed558ccdull + at * 0xc4ceb9fe1a85ec53ull + salt);
    }
};

// the salt of an array by its place in the call's list: Variable arrays (place 0: the first) and arrays of scalars; then the other
// three arrays of a weighted sum
constexpr unsigned long long kSaltStep = 0x9e3779b97f4a7c15ull;
PG_DIGEST_HD unsigned long long var_array_salt(unsigned place) { return 0x243f6a8885a308d3ull + (place + 1) * kSaltStep; }
PG_DIGEST_HD unsigned long long scalar_array_salt(unsigned place) { return 0x13198a2e03707344ull + place * kSaltStep; }
constexpr unsigned long long kSaltSegOff = 0x452821e638d01377ull, kSaltCoeff = 0xbe5466cf34e90c6cull, kSaltConstant = 0xc0ac29b7c97c50ddull;

// The result block of one preflight: on the device the passes accumulate into it, the host reads a copy.  It starts as zeros, but
// for the leading words of `call` that a call declares as "first offender" (atomicMin: they start at ~0).
struct Preflight {
    unsigned long long max_var;  // the largest entry of the Variable arrays
    Digest vars;                 // the Variable arrays
    Digest others;               // the call's other device arrays (bounds, offsets, coefficients, constants)
    unsigned long long call[3];  // the call's own words: first offenders and counts (each call's kernel names them; unnamed: unread)
};
static_assert(sizeof(Preflight) == 64, "the preflight's result block is one 64-byte copy");

#if defined(__HIPCC__)
// the end of a digesting kernel: the wave's sum, added to *out by lane 0
__device__ __forceinline__ void digest_flush(const Digest &lane, Digest *out) {
    unsigned long long h1 = lane.h1, h2 = lane.h2;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        h1 += __shfl_xor(h1, d, 64);
        h2 += __shfl_xor(h2, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out->h1, h1);
        atomicAdd(&out->h2, h2);
    }
}
#endif

}  // namespace pg
