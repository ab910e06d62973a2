// capi_open.inc -- the opening entry points of the C ABI (pg_poly_open, pg_poly_combine), included at the end of capi.hip:
// host-side validation, workspace and kernel launches of opening.hpp.  DESIGN section 3.12.
#include "opening.hpp"

namespace {

pg::Fr fr_pow_u64(pg::Fr x, uint64_t k) {
    pg::Fr r = pg::fr_one();
    for (; k; k >>= 1, x = pg::fr_mul(x, x))
        if (k & 1) r = pg::fr_mul(r, x);
    return r;
}

// the checks both calls share; fills A's columns, weights and sizes.  `outs` are the output ranges (bytes) that may overlap
// no input column.
pg_status open_prepare(pg_engine *e, const pg_scalar *const *d_cols, const pg_scalar *mu, uint64_t n_cols, uint64_t n,
                       std::initializer_list<std::pair<const void *, uint64_t>> outs, pg::OpenArgs &A) {
    if (!e || !d_cols || !mu) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_cols < 1 || n_cols > pg::kOpenMaxCols) return fail(PG_ERR_INVALID_ARGUMENT, "n_cols must be in [1, 32]");
    if (n == 0 || n > (1ull << 32)) return fail(PG_ERR_INVALID_ARGUMENT, "n must be in [1, 2^32]");
    const uint64_t col_bytes = n * sizeof(pg_scalar);
    for (const auto &o : outs) PG_TRY(check_scalars(o.first, "an output"));
    for (uint64_t j = 0; j < n_cols; j++) {
        PG_TRY(check_scalars(d_cols[j], "d_cols[j]"));
        PG_TRY(check_field(&mu[j], "mu[j]"));
        for (const auto &o : outs)
            if (overlaps(o.first, o.second, d_cols[j], col_bytes)) return fail(PG_ERR_INVALID_ARGUMENT, "an output overlaps an input column");
        A.col[j] = reinterpret_cast<const uint4 *>(d_cols[j]);
        A.mu[j] = to_fr(&mu[j]);
        if (pg::fr_eq(A.mu[j], pg::fr_one())) A.one_mask |= 1u << j;
    }
    for (uint64_t j = n_cols; j < pg::kOpenMaxCols; j++) A.col[j] = A.col[0];
    A.n_cols = (uint32_t)n_cols;
    A.n = n;
    A.tiles = (n + pg::kOpenTile - 1) / pg::kOpenTile;
    return PG_OK;
}

}  // namespace

extern "C" {

pg_status pg_poly_open(pg_engine *e, const pg_scalar *const *d_cols, const pg_scalar *mu, uint64_t n_cols, uint64_t n,
                       const pg_scalar *point, pg_scalar *d_witness, pg_scalar *d_value, void *stream) {
    pg::OpenArgs A{};
    PG_TRY(check_field(point, "point"));
    PG_TRY(open_prepare(e, d_cols, mu, n_cols, n, {{d_witness, n * sizeof(pg_scalar)}, {d_value, sizeof(pg_scalar)}}, A));
    if (overlaps(d_witness, n * sizeof(pg_scalar), d_value, sizeof(pg_scalar)))
        return fail(PG_ERR_INVALID_ARGUMENT, "d_value overlaps d_witness");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    PG_TRY(e->d_open.carve(16, [&](Carve cv) {
        A.tot = cv.take<uint4>(2 * A.tiles);
        return cv.bytes();
    }));
    A.f = reinterpret_cast<uint4 *>(d_witness);
    A.value = reinterpret_cast<uint4 *>(d_value);
    A.chunk = (A.tiles + pg::kThreads - 1) / pg::kThreads;
    A.xpow2[0] = to_fr(point);
    for (int b = 1; b < 12; b++) A.xpow2[b] = pg::fr_mul(A.xpow2[b - 1], A.xpow2[b - 1]);
    A.chunk_pow[0] = fr_pow_u64(A.xpow2[11], A.chunk);
    for (int k = 1; k < 8; k++) A.chunk_pow[k] = pg::fr_mul(A.chunk_pow[k - 1], A.chunk_pow[k - 1]);
    const uint64_t cap1 = (uint64_t)e->num_cus * 8, cap3 = (uint64_t)e->num_cus * 2;  // (pass 3: 68 KiB of LDS, two per CU)
    hipLaunchKernelGGL(pg::open_combine_kernel<true>, dim3(grid_cap(A.tiles, cap1)), dim3(pg::kThreads), 0, st, A);
    hipLaunchKernelGGL(pg::open_carry_kernel, dim3(1), dim3(pg::kThreads), 0, st, A);
    hipLaunchKernelGGL(pg::open_quotient_kernel, dim3(grid_cap(A.tiles, cap3)), dim3(pg::kThreads), 0, st, A);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_poly_combine(pg_engine *e, const pg_scalar *const *d_cols, const pg_scalar *mu, uint64_t n_cols, uint64_t n,
                          pg_scalar *d_out, void *stream) {
    pg::OpenArgs A{};
    PG_TRY(open_prepare(e, d_cols, mu, n_cols, n, {{d_out, n * sizeof(pg_scalar)}}, A));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    A.f = reinterpret_cast<uint4 *>(d_out);
    const uint64_t cap = (uint64_t)e->num_cus * 8;
    hipLaunchKernelGGL(pg::open_combine_kernel<false>, dim3(grid_cap(A.tiles, cap)), dim3(pg::kThreads), 0, st, A);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

}  // extern "C"
