// host_util.hpp -- what the host side of the C ABI (capi.hip and its capi_*.inc) shares: workspace layouts (Carve), the
// owners of everything allocated or created (owners.hpp), status plumbing and argument checks.  Included by capi.hip alone,
// before anything that uses it.  The first part needs no HIP: a plain host compiler sees it alone (tests/cpp/carve_host.cpp, g++).
#pragma once

#include <cstdint>

namespace pg {

inline uint64_t round256(uint64_t b) { return (b + 255) / 256 * 256; }

// A workspace layout: ONE sequence of take<T>(count) calls, run twice -- first with no base, to measure (bytes() is then the
// size to reserve), then against the reserved buffer, to place.  Every part starts on a multiple of `align` bytes from the base
// and a part of count 0 takes no room.  Offsets only: the measuring pass hands out nullptr, never arithmetic on it.
class Carve {
  public:
    explicit Carve(uint64_t align, void *base = nullptr) : base_(static_cast<char *>(base)), align_(align) {}
    template <typename T>
    T *take(uint64_t count) {
        const uint64_t at = off_;
        off_ += (count * sizeof(T) + align_ - 1) / align_ * align_;
        return base_ ? reinterpret_cast<T *>(base_ + at) : nullptr;
    }
    uint64_t bytes() const { return off_; }

  private:
    char *base_;
    uint64_t align_, off_ = 0;
};

}  // namespace pg

#if defined(__HIPCC__)  // the rest needs the HIP runtime and the C ABI's types

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/plonk_gadgets_hip.h"
#include "fr.hpp"
#include "owners.hpp"  // fail, PG_TRY, PG_HIP_TRY; Scratch, Pinned, Event, Stream, Staging, CallBuffers, ColumnStore

namespace {

using pg::round256;

inline pg::Fr to_fr(const pg_scalar *s) {
    pg::Fr f;
    std::memcpy(f.l, s->l, sizeof f.l);
    return f;
}
inline void from_fr(const pg::Fr &f, pg_scalar *out) { std::memcpy(out->l, f.l, sizeof f.l); }

inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// a BlsScalar is always fully reduced; reject limbs >= q instead of computing garbage
bool is_reduced(const pg::Fr &f) {
    const uint64_t Q[4] = {PG_Q0, PG_Q1, PG_Q2, PG_Q3};
    for (int i = 3; i >= 0; i--) {
        if (f.l[i] < Q[i]) return true;
        if (f.l[i] > Q[i]) return false;
    }
    return false;
}

pg_status check_scalars(const void *p, const char *what) {
    if (!p || !aligned(p, 16)) return fail(PG_ERR_INVALID_ARGUMENT, std::string(what) + " NULL or not 16-byte aligned");
    return PG_OK;
}
pg_status check_u64s(const void *p, const char *what, bool nullable = false) {
    if (!p && nullable) return PG_OK;
    if (!p || !aligned(p, 8)) return fail(PG_ERR_INVALID_ARGUMENT, std::string(what) + " NULL or not 8-byte aligned");
    return PG_OK;
}

pg_status check_field(const pg_scalar *s, const char *what) {
    if (!s) return fail(PG_ERR_INVALID_ARGUMENT, std::string(what) + " is NULL");
    if (!is_reduced(to_fr(s))) return fail(PG_ERR_INVALID_ARGUMENT, std::string(what) + " is not reduced below the modulus");
    return PG_OK;
}

// n_cols columns of n scalars, col_stride scalars apart (n >= 1)
pg_status check_strided_columns(uint64_t n, uint64_t n_cols, uint64_t col_stride) {
    if (col_stride < n) return fail(PG_ERR_INVALID_ARGUMENT, "col_stride < n");
    if (n_cols && (n_cols - 1) > (UINT64_MAX / sizeof(pg_scalar) - n) / col_stride)
        return fail(PG_ERR_INVALID_ARGUMENT, "n_cols x col_stride overflows the address space");
    return PG_OK;
}

bool overlaps(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}

// pw[b] = base^(2^b): the table PpPowers::pw and FrPow2::pw carry to the kernels
void fill_squares(pg::Fr (&pw)[32], const pg::Fr &base) {
    pw[0] = base;
    for (int b = 1; b < 32; b++) pw[b] = pg::fr_mul(pw[b - 1], pw[b - 1]);
}

uint32_t grid_for_lanes(uint64_t lanes, uint32_t threads) { return (uint32_t)((lanes + threads - 1) / threads); }

// a launch of `want` workgroups, at most `cap` of them (the kernel loops over the rest)
uint32_t grid_cap(uint64_t want, uint64_t cap) { return (uint32_t)(want < cap ? want : cap); }

}  // namespace

#endif  // __HIPCC__
