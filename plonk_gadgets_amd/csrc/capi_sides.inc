// capi_sides.inc -- pg_plonk_sides, pg_plonk_range_sides and their host-only forms, included at the end of capi.hip after
// capi_codec.inc: host-side validation, the workspace and the two launches of plonk_sides.hpp.  DESIGN sections 3.16 and 3.21.
#include "plonk_sides.hpp"

namespace {

static_assert(sizeof(pg_plonk_key) == sizeof(pg::PlonkKey) && offsetof(pg_plonk_key, pos) == offsetof(pg::PlonkKey, pos) &&
                  offsetof(pg_plonk_key, omega) == offsetof(pg::PlonkKey, omega) &&
                  offsetof(pg_plonk_key, points) == offsetof(pg::PlonkKey, points) && offsetof(pg_plonk_key, g) == offsetof(pg::PlonkKey, g),
              "pg_plonk_key is pg::PlonkKey");
static_assert(sizeof(pg_plonk_range_key) == sizeof(pg::PlonkRangeKey) && sizeof(pg_plonk_range_key) == 1488 &&
                  offsetof(pg_plonk_range_key, state) == 0 && offsetof(pg_plonk_range_key, pos) == offsetof(pg_plonk_key, pos) &&
                  offsetof(pg_plonk_range_key, log2_n) == offsetof(pg_plonk_key, log2_n) &&
                  offsetof(pg_plonk_range_key, omega) == offsetof(pg_plonk_key, omega) &&
                  offsetof(pg_plonk_range_key, points) == offsetof(pg_plonk_key, points) &&
                  offsetof(pg_plonk_range_key, g) == offsetof(pg_plonk_key, g) &&
                  offsetof(pg_plonk_range_key, q_range) == sizeof(pg_plonk_key) &&
                  offsetof(pg::PlonkRangeKey, q_range) == sizeof(pg_plonk_key),
              "pg_plonk_range_key is a pg_plonk_key followed by q_range: pg::PlonkRangeKey");
static_assert(PG_SIDES_OK == pg::kSidesOk && PG_SIDES_BAD_EVALUATION == pg::kSidesBadEvaluation &&
                  PG_SIDES_XI_IN_DOMAIN == pg::kSidesXiInDomain && PG_SIDES_BAD_PUBLIC_INPUT == pg::kSidesBadPublicInput &&
                  PG_SIDES_BAD_KEY == pg::kSidesBadKey && PG_PLONK_PROOF_BYTES == pg::kProofBytes && PG_PLONK_SIDES_ROWS == pg::kSidesRows &&
                  PG_PLONK_RANGE_SIDES_ROWS == pg::kSidesRangeRows,
              "the header's values are plonk_sides.hpp's");

// what differs between the table of 23 rows and the one of 24: the messages (n x rows must stay below pg_msm_segmented's 2^31)
template <bool RANGE>
struct SidesCall {
    static constexpr uint32_t kRows = pg::SidesTable<RANGE>::kRows;
    static constexpr uint64_t kMaxProofs = ((1ull << 31) - 1) / kRows;
    static constexpr const char *kTooMany = RANGE ? "n x 24 rows must be below 2^31" : "n x 23 rows must be below 2^31";
    static constexpr const char *kStride = RANGE ? "col_stride < 24 n" : "col_stride < 23 n";
};

template <bool RANGE>
pg_status plonk_sides_device(pg_engine *e, const uint8_t *d_proofs, uint64_t n, const typename pg::SidesTable<RANGE>::Record *d_keys,
                             uint64_t n_keys, const uint32_t *d_key_index, const uint64_t *d_pi_off, const uint64_t *d_pi_rows,
                             const pg_scalar *d_pi_vals, pg_g1_affine *d_bases, pg_scalar *d_scalars, uint64_t col_stride, uint8_t *d_status,
                             uint8_t *d_where, void *stream) {
    using Call = SidesCall<RANGE>;
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n == 0) return PG_OK;
    if (n > Call::kMaxProofs) return fail(PG_ERR_INVALID_ARGUMENT, Call::kTooMany);
    if (n_keys == 0 || n_keys > (1ull << 32)) return fail(PG_ERR_INVALID_ARGUMENT, "n_keys must be in [1, 2^32]");
    PG_TRY(check_scalars(d_proofs, "d_proofs"));
    PG_TRY(check_scalars(d_keys, "d_keys"));
    PG_TRY(check_scalars(d_bases, "d_bases"));
    PG_TRY(check_scalars(d_scalars, "d_scalars"));
    if (d_key_index && !aligned(d_key_index, 4)) return fail(PG_ERR_INVALID_ARGUMENT, "d_key_index not 4-byte aligned");
    if (d_pi_off) {
        PG_TRY(check_u64s(d_pi_off, "d_pi_off"));
        PG_TRY(check_u64s(d_pi_rows, "d_pi_rows"));
        PG_TRY(check_scalars(d_pi_vals, "d_pi_vals"));
    }
    if (!d_status || !d_where) return fail(PG_ERR_INVALID_ARGUMENT, "d_status or d_where NULL");
    const uint64_t rows = n * Call::kRows;
    if (col_stride < rows) return fail(PG_ERR_INVALID_ARGUMENT, Call::kStride);
    if (col_stride > (UINT64_MAX / sizeof(pg_scalar) - rows)) return fail(PG_ERR_INVALID_ARGUMENT, "col_stride overflows the address space");
    // every output against every other and against every input whose size the host knows
    const struct { const void *p; uint64_t bytes; } outs[4] = {{d_bases, rows * sizeof(pg_g1_affine)},
                                                               {d_scalars, (col_stride + rows) * sizeof(pg_scalar)},
                                                               {d_status, n},
                                                               {d_where, n}},
                                                    ins[4] = {{d_proofs, n * pg::kProofBytes},
                                                              {d_keys, n_keys * sizeof(*d_keys)},
                                                              {d_key_index, d_key_index ? 4 * n : 0},
                                                              {d_pi_off, d_pi_off ? 8 * (n + 1) : 0}};
    for (int a = 0; a < 4; a++) {
        for (int b = a + 1; b < 4; b++)
            if (overlaps(outs[a].p, outs[a].bytes, outs[b].p, outs[b].bytes)) return fail(PG_ERR_INVALID_ARGUMENT, "two outputs overlap");
        for (int b = 0; b < 4; b++)
            if (ins[b].bytes && overlaps(outs[a].p, outs[a].bytes, ins[b].p, ins[b].bytes))
                return fail(PG_ERR_INVALID_ARGUMENT, "an output overlaps an input");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    // workspace: the decode status of every commitment
    uint8_t *cstat;
    PG_TRY(e->d_sides.carve(16, [&](Carve cv) {
        cstat = cv.take<uint8_t>(n * pg::kSidesCommitments);
        return cv.bytes();
    }));
    pg::G1A *bases = reinterpret_cast<pg::G1A *>(d_bases);
    hipLaunchKernelGGL(pg::plonk_sides_decode_kernel, dim3(grid_of(e, n * pg::kSidesCommitments, 8)), dim3(pg::kThreads), 0, st, d_proofs, n,
                       Call::kRows, bases, cstat);
    const dim3 grid(grid_for_lanes(n, pg::kSidesLanes)), block(pg::kSidesLanes);
    const pg::Fr *pi_vals = reinterpret_cast<const pg::Fr *>(d_pi_vals);
    pg::Fr *scalars = reinterpret_cast<pg::Fr *>(d_scalars);
    if constexpr (RANGE)
        hipLaunchKernelGGL(pg::plonk_range_sides_kernel, grid, block, 0, st, d_proofs, n, d_keys, n_keys, d_key_index, d_pi_off, d_pi_rows,
                           pi_vals, cstat, bases, scalars, col_stride, d_status, d_where);
    else
        hipLaunchKernelGGL(pg::plonk_sides_kernel, grid, block, 0, st, d_proofs, n, d_keys, n_keys, d_key_index, d_pi_off, d_pi_rows, pi_vals,
                           cstat, bases, scalars, col_stride, d_status, d_where);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

template <bool RANGE>
pg_status plonk_sides_on_host(const uint8_t *proofs, uint64_t n, const typename pg::SidesTable<RANGE>::Record *keys, uint64_t n_keys,
                              const uint32_t *key_index, const uint64_t *pi_off, const uint64_t *pi_rows, const pg_scalar *pi_vals,
                              pg_g1_affine *bases, pg_scalar *scalars, uint64_t col_stride, uint8_t *status, uint8_t *where) {
    using Call = SidesCall<RANGE>;
    if (n == 0) return PG_OK;
    if (!proofs || !keys || !bases || !scalars || !status || !where) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > Call::kMaxProofs) return fail(PG_ERR_INVALID_ARGUMENT, Call::kTooMany);
    if (n_keys == 0) return fail(PG_ERR_INVALID_ARGUMENT, "n_keys = 0");
    if (col_stride < n * Call::kRows) return fail(PG_ERR_INVALID_ARGUMENT, Call::kStride);
    if (!aligned(keys, 8) || !aligned(bases, 8) || !aligned(scalars, 8) || (key_index && !aligned(key_index, 4)))
        return fail(PG_ERR_INVALID_ARGUMENT, "a pointer is not aligned to its element");
    if (pi_off && (!pi_rows || !pi_vals || !aligned(pi_off, 8) || !aligned(pi_rows, 8) || !aligned(pi_vals, 8)))
        return fail(PG_ERR_INVALID_ARGUMENT, "pi_rows or pi_vals NULL or misaligned");
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *proof = proofs + i * pg::kProofBytes;
        pg::G1A *rows = reinterpret_cast<pg::G1A *>(bases) + i * Call::kRows;
        uint8_t cstat[pg::kSidesCommitments];
        for (uint32_t j = 0; j < pg::kSidesCommitments; j++) {
            pg::G1Bytes b;
            std::memcpy(b.w, proof + 48 * j, 48);
            cstat[j] = pg::g1_decode(b, true, rows + j);
        }
        uint32_t mem[pg::kSidesWords];
        pg::Fr *sa = reinterpret_cast<pg::Fr *>(scalars) + i * Call::kRows;
        pg::plonk_sides_one<1, RANGE>(proof, keys, n_keys, key_index ? key_index[i] : 0u, pi_rows, reinterpret_cast<const pg::Fr *>(pi_vals),
                                      pi_off ? pi_off[i] : 0, pi_off ? pi_off[i + 1] : 0, cstat, mem, rows, sa, sa + col_stride, status + i,
                                      where + i);
    }
    return PG_OK;
}

}  // namespace

extern "C" {

pg_status pg_plonk_sides(pg_engine *e, const uint8_t *d_proofs, uint64_t n, const pg_plonk_key *d_keys, uint64_t n_keys,
                         const uint32_t *d_key_index, const uint64_t *d_pi_off, const uint64_t *d_pi_rows, const pg_scalar *d_pi_vals,
                         pg_g1_affine *d_bases, pg_scalar *d_scalars, uint64_t col_stride, uint8_t *d_status, uint8_t *d_where,
                         void *stream) {
    return plonk_sides_device<false>(e, d_proofs, n, reinterpret_cast<const pg::PlonkKey *>(d_keys), n_keys, d_key_index, d_pi_off, d_pi_rows,
                                     d_pi_vals, d_bases, d_scalars, col_stride, d_status, d_where, stream);
}

pg_status pg_plonk_sides_host(const uint8_t *proofs, uint64_t n, const pg_plonk_key *keys, uint64_t n_keys, const uint32_t *key_index,
                              const uint64_t *pi_off, const uint64_t *pi_rows, const pg_scalar *pi_vals, pg_g1_affine *bases,
                              pg_scalar *scalars, uint64_t col_stride, uint8_t *status, uint8_t *where) {
    return plonk_sides_on_host<false>(proofs, n, reinterpret_cast<const pg::PlonkKey *>(keys), n_keys, key_index, pi_off, pi_rows, pi_vals,
                                      bases, scalars, col_stride, status, where);
}

pg_status pg_plonk_range_sides(pg_engine *e, const uint8_t *d_proofs, uint64_t n, const pg_plonk_range_key *d_keys, uint64_t n_keys,
                               const uint32_t *d_key_index, const uint64_t *d_pi_off, const uint64_t *d_pi_rows, const pg_scalar *d_pi_vals,
                               pg_g1_affine *d_bases, pg_scalar *d_scalars, uint64_t col_stride, uint8_t *d_status, uint8_t *d_where,
                               void *stream) {
    return plonk_sides_device<true>(e, d_proofs, n, reinterpret_cast<const pg::PlonkRangeKey *>(d_keys), n_keys, d_key_index, d_pi_off,
                                    d_pi_rows, d_pi_vals, d_bases, d_scalars, col_stride, d_status, d_where, stream);
}

pg_status pg_plonk_range_sides_host(const uint8_t *proofs, uint64_t n, const pg_plonk_range_key *keys, uint64_t n_keys,
                                    const uint32_t *key_index, const uint64_t *pi_off, const uint64_t *pi_rows, const pg_scalar *pi_vals,
                                    pg_g1_affine *bases, pg_scalar *scalars, uint64_t col_stride, uint8_t *status, uint8_t *where) {
    return plonk_sides_on_host<true>(proofs, n, reinterpret_cast<const pg::PlonkRangeKey *>(keys), n_keys, key_index, pi_off, pi_rows,
                                     pi_vals, bases, scalars, col_stride, status, where);
}

}  // extern "C"
