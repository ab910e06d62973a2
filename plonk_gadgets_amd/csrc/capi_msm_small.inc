// capi_msm_small.inc -- pg_msm_segmented, included at the end of capi.hip: host-side validation, workspace and the launches of
// msm_small.hpp.  DESIGN section 3.15.
#include "emit.hpp"  // kThreads
#include "msm.hpp"   // g1_normalize_kernel, kNormPerLane
#include "msm_small.hpp"

namespace {

// the segment offsets travel through a pinned buffer of the engine, so the copy is asynchronous and the caller's array is
// free when the call returns; the buffer is rewritten only once the copy of the call before has left it
pg_status stage_offsets(pg_engine *e, const uint64_t *seg_off, uint64_t count, uint64_t *d_off, hipStream_t st) {
    PG_TRY(e->seg.acquire((count < 1024 ? 1024 : count) * sizeof(uint64_t), false));
    std::memcpy(e->seg.host(), seg_off, count * sizeof(uint64_t));
    PG_HIP_TRY(hipMemcpyAsync(d_off, e->seg.host(), count * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    PG_HIP_TRY(e->seg.sent(st));
    return PG_OK;
}

}  // namespace

extern "C" {

pg_status pg_msm_segmented(pg_engine *e, const pg_g1_affine *d_bases, const pg_scalar *d_scalars, uint64_t n, uint64_t n_cols,
                           uint64_t col_stride, const uint64_t *seg_off, uint64_t n_segs, pg_g1_affine *d_out, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_segs == 0) return PG_OK;
    PG_TRY(check_scalars(d_bases, "d_bases"));
    PG_TRY(check_scalars(d_scalars, "d_scalars"));
    PG_TRY(check_scalars(d_out, "d_out"));
    if (!seg_off) return fail(PG_ERR_INVALID_ARGUMENT, "seg_off is NULL");
    if (n == 0) return fail(PG_ERR_INVALID_ARGUMENT, "n = 0 with segments to sum");
    if (n_cols == 0) return fail(PG_ERR_INVALID_ARGUMENT, "n_cols = 0");
    if (n >= (1ull << 31) || n_cols >= (1ull << 31) || n * n_cols >= (1ull << 31))
        return fail(PG_ERR_INVALID_ARGUMENT, "n x n_cols must be below 2^31");
    if (n_segs >= (1ull << 31) || n_segs * n_cols >= (1ull << 31))
        return fail(PG_ERR_INVALID_ARGUMENT, "n_segs x n_cols must be below 2^31");
    PG_TRY(check_strided_columns(n, n_cols, col_stride));
    if (seg_off[0] != 0 || seg_off[n_segs] != n) return fail(PG_ERR_INVALID_ARGUMENT, "seg_off must start at 0 and end at n");
    for (uint64_t k = 0; k < n_segs; k++)
        if (seg_off[k] > seg_off[k + 1]) return fail(PG_ERR_INVALID_ARGUMENT, "seg_off decreases");
    const uint64_t lanes = n * n_cols, sums = n_segs * n_cols, out_bytes = sums * sizeof(pg_g1_affine);
    if (overlaps(d_out, out_bytes, d_bases, n * sizeof(pg_g1_affine)) ||
        overlaps(d_out, out_bytes, d_scalars, ((n_cols - 1) * col_stride + n) * sizeof(pg_scalar)))
        return fail(PG_ERR_INVALID_ARGUMENT, "d_out overlaps an input");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    // workspace: the products, the segments' sums (both XYZZ) and the offsets
    pg::G1X *prod, *res;
    uint64_t *d_off;
    PG_TRY(e->d_msm_small.carve(256, [&](Carve cv) {
        prod = cv.take<pg::G1X>(lanes);
        res = cv.take<pg::G1X>(sums);
        d_off = cv.take<uint64_t>(n_segs + 1);
        return cv.bytes();
    }));
    PG_TRY(stage_offsets(e, seg_off, n_segs + 1, d_off, st));
    hipLaunchKernelGGL(pg::msm_seg_mul_kernel, dim3(grid_for_lanes(lanes, pg::kSmallLanes)), dim3(pg::kSmallLanes), 0, st,
                       reinterpret_cast<const pg::G1A *>(d_bases), reinterpret_cast<const pg::Fr *>(d_scalars), n, n_cols, col_stride,
                       prod);
    const uint64_t sum_cap = (uint64_t)e->num_cus * 32;  // waves of the sums resident at once, about; the kernel walks the rest
    hipLaunchKernelGGL(pg::msm_seg_sum_kernel, dim3(grid_cap(sums, sum_cap)), dim3(pg::kSmallLanes), 0, st, prod,
                       d_off, n, n_segs, n_cols, res);
    // one inversion per lane: a lane takes up to kNormPerLane sums once there are enough of them to fill the device
    const uint64_t norm_lanes = (uint64_t)e->num_cus * pg::kThreads;
    uint64_t per_lane = (sums + norm_lanes - 1) / norm_lanes;
    if (per_lane > pg::kNormPerLane) per_lane = pg::kNormPerLane;
    hipLaunchKernelGGL(pg::g1_normalize_kernel, dim3(grid_for_lanes((sums + per_lane - 1) / per_lane, pg::kThreads)), dim3(pg::kThreads),
                       0, st, res, reinterpret_cast<pg::G1A *>(d_out), sums, (uint32_t)per_lane);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

}  // extern "C"
