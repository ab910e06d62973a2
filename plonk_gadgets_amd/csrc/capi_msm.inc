// capi_msm.inc -- the commitment entry points of the C ABI (pg_msm, pg_srs_setup, pg_g1_to_compressed), included at the end of
// capi.hip: host-side validation, workspace and kernel launches of msm.hpp.  DESIGN section 3.11.
#include "msm.hpp"

namespace {

static_assert(sizeof(pg_g1_affine) == sizeof(pg::G1A), "pg_g1_affine is pg::G1A");

inline pg::G1A to_g1a(const pg_g1_affine *p) {
    pg::G1A a;
    std::memcpy(a.x.l, p->x, sizeof a.x.l);
    std::memcpy(a.y.l, p->y, sizeof a.y.l);
    return a;
}

}  // namespace

extern "C" {

pg_status pg_msm(pg_engine *e, const pg_g1_affine *d_bases, const pg_scalar *d_scalars, uint64_t n, uint64_t n_cols,
                 uint64_t col_stride, pg_g1_affine *d_out, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_scalars(d_bases, "d_bases"));
    PG_TRY(check_scalars(d_scalars, "d_scalars"));
    PG_TRY(check_scalars(d_out, "d_out"));
    if (n == 0 || n >= (1ull << 31)) return fail(PG_ERR_INVALID_ARGUMENT, "n must be in [1, 2^31)");
    PG_TRY(check_strided_columns(n, n_cols, col_stride));
    if (n_cols == 0) return PG_OK;
    const uint64_t out_bytes = n_cols * sizeof(pg_g1_affine);
    if (overlaps(d_out, out_bytes, d_bases, n * sizeof(pg_g1_affine)) ||
        overlaps(d_out, out_bytes, d_scalars, ((n_cols - 1) * col_stride + n) * sizeof(pg_scalar)))
        return fail(PG_ERR_INVALID_ARGUMENT, "d_out overlaps an input");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    // workspace: sort keys / values (two of each), the sort's temporary storage, two levels of partials, buckets, sums
    size_t sort_bytes = 0;
    {
        uint64_t *nul = nullptr;
        PG_HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_bytes, nul, nul, (size_t)n, 32u, 48u, st));
    }
    const uint64_t lanes0 = (n + pg::kMsmRun - 1) / pg::kMsmRun, partA = 2 * lanes0,
                   partB = 2 * ((partA + pg::kMsmRun - 1) / pg::kMsmRun);
    const uint64_t nbk = (uint64_t)pg::kMsmWindows * (pg::kMsmBuckets + 1), nseg = (uint64_t)pg::kMsmWindows * pg::kMsmSegs;
    uint64_t *k0, *k1;
    void *sort_tmp;
    uint32_t *pkA, *pkB;
    pg::G1X *ppA, *ppB, *buckets, *seg, *win, *res;
    PG_TRY(e->d_msm.carve(256, [&](Carve cv) {
        k0 = cv.take<uint64_t>(n);
        k1 = cv.take<uint64_t>(n);
        sort_tmp = cv.take<char>(sort_bytes);
        pkA = cv.take<uint32_t>(partA);
        ppA = cv.take<pg::G1X>(partA);
        pkB = cv.take<uint32_t>(partB);
        ppB = cv.take<pg::G1X>(partB);
        buckets = cv.take<pg::G1X>(nbk);
        seg = cv.take<pg::G1X>(nseg);
        win = cv.take<pg::G1X>(pg::kMsmWindows);
        res = cv.take<pg::G1X>(n_cols);
        return cv.bytes();
    }));
    const pg::G1A *bases = reinterpret_cast<const pg::G1A *>(d_bases);
    const uint32_t dgrid = grid_of(e, n, 8);
    for (uint64_t j = 0; j < n_cols; j++) {
        const pg::Fr *s = reinterpret_cast<const pg::Fr *>(d_scalars + j * col_stride);
        PG_HIP_TRY(hipMemsetAsync(buckets, 0, nbk * sizeof(pg::G1X), st));  // ZZ = 0: the identity
        for (uint32_t w = 0; w < pg::kMsmWindows; w++) {
            pg::G1X *bw = buckets + (uint64_t)w * (pg::kMsmBuckets + 1);
            hipLaunchKernelGGL(pg::msm_digits_kernel, dim3(dgrid), dim3(pg::kThreads), 0, st, s, n, w, k0);
            size_t tb = sort_bytes;
            PG_HIP_TRY(rocprim::radix_sort_keys(sort_tmp, tb, k0, k1, (size_t)n, 32u, 48u, st));
            uint64_t lanes = lanes0;
            hipLaunchKernelGGL(pg::msm_segsum_kernel<true>, dim3(grid_for_lanes(lanes, pg::kThreads)), dim3(pg::kThreads), 0, st,
                               k1, nullptr, bases, nullptr, n, bw, pkA, ppA);
            // further levels over the partials (2 per lane of the level before) until one lane held everything
            uint32_t *ik = pkA, *ok = pkB;
            pg::G1X *ip = ppA, *op = ppB;
            while (lanes > 1) {
                const uint64_t m = 2 * lanes;
                lanes = (m + pg::kMsmRun - 1) / pg::kMsmRun;
                hipLaunchKernelGGL(pg::msm_segsum_kernel<false>, dim3(grid_for_lanes(lanes, pg::kThreads)), dim3(pg::kThreads), 0, st,
                                   nullptr, ik, nullptr, ip, m, bw, ok, op);
                std::swap(ik, ok);
                std::swap(ip, op);
            }
        }
        hipLaunchKernelGGL(pg::msm_bucket_reduce_kernel, dim3(grid_for_lanes(nseg, pg::kMsmSmallThreads)), dim3(pg::kMsmSmallThreads),
                           0, st, buckets, seg);
        hipLaunchKernelGGL(pg::msm_window_kernel, dim3(1), dim3(pg::kMsmSmallThreads), 0, st, seg, win);
        hipLaunchKernelGGL(pg::msm_combine_kernel, dim3(1), dim3(pg::kMsmSmallThreads), 0, st, win, res + j);
    }
    hipLaunchKernelGGL(pg::g1_normalize_kernel, dim3(grid_for_lanes(n_cols, pg::kThreads)), dim3(pg::kThreads), 0, st, res,
                       reinterpret_cast<pg::G1A *>(d_out), n_cols, 1u);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_srs_setup(pg_engine *e, const pg_scalar *tau, const pg_g1_affine *base, uint64_t n, pg_g1_affine *d_out, void *stream) {
    if (!e || !tau) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_field(tau, "tau"));
    PG_TRY(check_scalars(d_out, "d_out"));
    if (n == 0 || n > (1ull << 32)) return fail(PG_ERR_INVALID_ARGUMENT, "n must be in [1, 2^32]");
    const pg::Fr t = to_fr(tau);
    if (pg::fr_is_zero(t)) return fail(PG_ERR_INVALID_ARGUMENT, "tau = 0");
    const pg::G1A b = base ? to_g1a(base) : pg::g1_generator();
    if (!pg::fq_is_reduced(b.x) || !pg::fq_is_reduced(b.y)) return fail(PG_ERR_INVALID_ARGUMENT, "base coordinates not reduced");
    if (pg::g1a_is_identity(b)) return fail(PG_ERR_INVALID_ARGUMENT, "base is the identity");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    const uint64_t chunk = n < pg::kSrsChunk ? n : pg::kSrsChunk;
    pg::G1X *tx, *pts;
    pg::G1A *ta;
    PG_TRY(e->d_srs.carve(256, [&](Carve cv) {
        tx = cv.take<pg::G1X>(8192);
        ta = cv.take<pg::G1A>(8192);
        pts = cv.take<pg::G1X>(chunk);
        return cv.bytes();
    }));
    hipLaunchKernelGGL(pg::srs_table_kernel, dim3(8192 / pg::kThreads), dim3(pg::kThreads), 0, st, b, tx);
    hipLaunchKernelGGL(pg::g1_normalize_kernel, dim3(grid_for_lanes(8192 / pg::kNormPerLane, pg::kThreads)), dim3(pg::kThreads), 0, st,
                       tx, ta, (uint64_t)8192, pg::kNormPerLane);
    pg::FrPow2 P{};
    fill_squares(P.pw, t);
    pg::G1A *out = reinterpret_cast<pg::G1A *>(d_out);
    for (uint64_t start = 0; start < n; start += chunk) {
        const uint64_t count = n - start < chunk ? n - start : chunk;
        hipLaunchKernelGGL(pg::srs_points_kernel, dim3(grid_for_lanes((count + pg::kSrsPerLane - 1) / pg::kSrsPerLane, pg::kThreads)),
                           dim3(pg::kThreads), 0, st, ta, P, start, count, pts);
        hipLaunchKernelGGL(pg::g1_normalize_kernel, dim3(grid_for_lanes((count + pg::kNormPerLane - 1) / pg::kNormPerLane, pg::kThreads)),
                           dim3(pg::kThreads), 0, st, pts, out + start, count, pg::kNormPerLane);
    }
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_g1_to_compressed(const pg_g1_affine *in, uint64_t count, uint8_t *out) {
    if (count && (!in || !out)) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    // (p - 1) / 2
    const uint64_t H[6] = {0xdcff7fffffffd555ull, 0x0f55ffff58a9ffffull, 0xb39869507b587b12ull,
                           0xb23ba5c279c2895full, 0x258dd3db21a5d66bull, 0x0d0088f51cbff34dull};
    for (uint64_t k = 0; k < count; k++) {
        const pg::G1A a = to_g1a(in + k);
        if (!pg::fq_is_reduced(a.x) || !pg::fq_is_reduced(a.y)) return fail(PG_ERR_INVALID_ARGUMENT, "coordinates not reduced");
        uint8_t *o = out + 48 * k;
        if (pg::g1a_is_identity(a)) {
            std::memset(o, 0, 48);
            o[0] = 0xc0;
            continue;
        }
        const pg::Fq x = pg::fq_from_mont(a.x), y = pg::fq_from_mont(a.y);
        for (int i = 0; i < 48; i++) o[i] = (uint8_t)(x.l[5 - i / 8] >> (8 * (7 - i % 8)));
        bool greater = false;
        for (int i = 5; i >= 0; i--)
            if (y.l[i] != H[i]) {
                greater = y.l[i] > H[i];
                break;
            }
        o[0] |= 0x80;
        if (greater) o[0] |= 0x20;
    }
    return PG_OK;
}

}  // extern "C"
