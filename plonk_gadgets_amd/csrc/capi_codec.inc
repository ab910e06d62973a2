// capi_codec.inc -- the G1 ingestion entry points of the C ABI (pg_g1_decompress, pg_g1_check, pg_g1_compress and the host-only
// pg_g1_from_compressed, pg_g1_check_host), included at the end of capi.hip: host-side validation and the kernel launches of
// g1_codec.hpp.  DESIGN section 3.14.
#include "g1_codec.hpp"

namespace {

static_assert(PG_G1_OK == pg::kG1Ok && PG_G1_BAD_ENCODING == pg::kG1BadEncoding && PG_G1_NOT_ON_CURVE == pg::kG1NotOnCurve &&
                  PG_G1_NOT_IN_SUBGROUP == pg::kG1NotInSubgroup && PG_G1_NOT_REDUCED == pg::kG1NotReduced,
              "the header's status values are g1_codec.hpp's");

pg_status check_codec_count(uint64_t n) {
    if (n == 0 || n > (1ull << 32)) return fail(PG_ERR_INVALID_ARGUMENT, "n must be in [1, 2^32]");
    return PG_OK;
}

pg_status check_status_outputs(const uint8_t *d_status, const uint64_t *d_first_bad, uint64_t n) {
    if (!d_status) return fail(PG_ERR_INVALID_ARGUMENT, "d_status NULL");
    PG_TRY(check_u64s(d_first_bad, "d_first_bad"));
    if (overlaps(d_status, n, d_first_bad, 8)) return fail(PG_ERR_INVALID_ARGUMENT, "d_first_bad overlaps d_status");
    return PG_OK;
}

}  // namespace

extern "C" {

pg_status pg_g1_decompress(pg_engine *e, const uint8_t *d_in, uint64_t n, int check_subgroup, pg_g1_affine *d_out, uint8_t *d_status,
                           uint64_t *d_first_bad, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_scalars(d_in, "d_in"));
    PG_TRY(check_scalars(d_out, "d_out"));
    PG_TRY(check_codec_count(n));
    PG_TRY(check_status_outputs(d_status, d_first_bad, n));
    const uint64_t in_bytes = 48 * n, out_bytes = n * sizeof(pg_g1_affine);
    if (overlaps(d_out, out_bytes, d_in, in_bytes) || overlaps(d_status, n, d_in, in_bytes) || overlaps(d_status, n, d_out, out_bytes) ||
        overlaps(d_first_bad, 8, d_in, in_bytes) || overlaps(d_first_bad, 8, d_out, out_bytes))
        return fail(PG_ERR_INVALID_ARGUMENT, "an output overlaps the input or another output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    unsigned long long *fb = reinterpret_cast<unsigned long long *>(d_first_bad);
    hipLaunchKernelGGL(pg::g1_first_bad_init_kernel, dim3(1), dim3(64), 0, st, fb, (unsigned long long)n);
    hipLaunchKernelGGL(pg::g1_decompress_kernel, dim3(grid_of(e, n, 8)), dim3(pg::kThreads), 0, st, reinterpret_cast<const uint4 *>(d_in), n,
                       check_subgroup ? 1u : 0u, reinterpret_cast<pg::G1A *>(d_out), d_status, fb);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_g1_check(pg_engine *e, const pg_g1_affine *d_points, uint64_t n, uint8_t *d_status, uint64_t *d_first_bad, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_scalars(d_points, "d_points"));
    PG_TRY(check_codec_count(n));
    PG_TRY(check_status_outputs(d_status, d_first_bad, n));
    const uint64_t in_bytes = n * sizeof(pg_g1_affine);
    if (overlaps(d_status, n, d_points, in_bytes) || overlaps(d_first_bad, 8, d_points, in_bytes))
        return fail(PG_ERR_INVALID_ARGUMENT, "an output overlaps the input");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    unsigned long long *fb = reinterpret_cast<unsigned long long *>(d_first_bad);
    hipLaunchKernelGGL(pg::g1_first_bad_init_kernel, dim3(1), dim3(64), 0, st, fb, (unsigned long long)n);
    hipLaunchKernelGGL(pg::g1_check_kernel, dim3(grid_of(e, n, 8)), dim3(pg::kThreads), 0, st, reinterpret_cast<const pg::G1A *>(d_points), n,
                       d_status, fb);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_g1_compress(pg_engine *e, const pg_g1_affine *d_points, uint64_t n, uint8_t *d_out, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_scalars(d_points, "d_points"));
    PG_TRY(check_scalars(d_out, "d_out"));
    PG_TRY(check_codec_count(n));
    if (overlaps(d_out, 48 * n, d_points, n * sizeof(pg_g1_affine))) return fail(PG_ERR_INVALID_ARGUMENT, "d_out overlaps the input");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    hipLaunchKernelGGL(pg::g1_compress_kernel, dim3(grid_of(e, n, 8)), dim3(pg::kThreads), 0, st, reinterpret_cast<const pg::G1A *>(d_points), n,
                       reinterpret_cast<uint4 *>(d_out));
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_g1_from_compressed(const uint8_t *in, uint64_t count, pg_g1_affine *out, uint8_t *status) {
    if (count && (!in || !out || !status)) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t k = 0; k < count; k++) {
        pg::G1Bytes b;
        std::memcpy(b.w, in + 48 * k, 48);
        pg::G1A p;
        status[k] = pg::g1_decode(b, true, &p);
        std::memcpy(out[k].x, p.x.l, sizeof p.x.l);
        std::memcpy(out[k].y, p.y.l, sizeof p.y.l);
    }
    return PG_OK;
}

pg_status pg_g1_check_host(const pg_g1_affine *in, uint64_t count, uint8_t *status) {
    if (count && (!in || !status)) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t k = 0; k < count; k++) status[k] = pg::g1a_check(to_g1a(in + k));
    return PG_OK;
}

}  // extern "C"
