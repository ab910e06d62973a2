// capi_pairing.inc -- the pairing entry points of the C ABI (pg_g2_mul, pg_g2_to_compressed, pg_g2_prepare, pg_pairing_check,
// pg_pairing_gt), included at the end of capi.hip: host-side G2 (g2.hpp), validation and the launch of pairing.hpp's kernel.
// DESIGN section 3.13.
#include "pairing.hpp"

struct pg_g2_prepared {
    int device = -1;
    Scratch lines;  // kAteLines lines (pg::G2Line) on the device
};

namespace {

static_assert(sizeof(pg_g2_affine) == sizeof(pg::G2A), "pg_g2_affine is pg::G2A");
static_assert(sizeof(pg::G1A) == sizeof(pg::Fq2), "the kernel stages points in Fq2 slots");

inline pg::G2A to_g2a(const pg_g2_affine *p) {
    pg::G2A a;
    std::memcpy(&a, p, sizeof a);
    return a;
}

bool g2a_is_reduced(const pg::G2A &a) {
    return pg::fq_is_reduced(a.x.c0) && pg::fq_is_reduced(a.x.c1) && pg::fq_is_reduced(a.y.c0) && pg::fq_is_reduced(a.y.c1);
}

pg_status launch_pairing(pg_engine *e, const pg_g1_affine *d_points, const pg_g2_prepared *const *prepared, uint64_t n_checks,
                         uint64_t n_pairs, uint8_t *d_ok, uint64_t *d_gt, void *stream) {
    if (!e || !prepared) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_pairs == 0 || n_pairs > (uint64_t)pg::kPairMaxPairs) return fail(PG_ERR_INVALID_ARGUMENT, "n_pairs must be in [1, 8]");
    if (n_checks > (1ull << 31)) return fail(PG_ERR_INVALID_ARGUMENT, "n_checks must be <= 2^31");
    if (n_checks == 0) return PG_OK;
    PG_TRY(check_scalars(d_points, "d_points"));
    pg::PairingLines L{};
    for (uint64_t j = 0; j < n_pairs; j++) {
        if (!prepared[j] || !prepared[j]->lines.get()) return fail(PG_ERR_INVALID_ARGUMENT, "a prepared point is NULL");
        if (prepared[j]->device != e->device) return fail(PG_ERR_INVALID_ARGUMENT, "a prepared point lives on another device");
        L.q[j] = prepared[j]->lines.as<pg::G2Line>();
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    const uint32_t grid = (uint32_t)((n_checks + pg::kPairChecks - 1) / pg::kPairChecks);
    hipLaunchKernelGGL(pg::pairing_check_kernel, dim3(grid), dim3(pg::kPairThreads), 0, st, reinterpret_cast<const pg::G1A *>(d_points), L,
                       n_checks, (uint32_t)n_pairs, d_ok, reinterpret_cast<pg::Fq2 *>(d_gt));
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

}  // namespace

extern "C" {

pg_status pg_g2_mul(const pg_g2_affine *p, const pg_scalar *k, pg_g2_affine *out) {
    if (!k || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_field(k, "k"));
    const pg::G2A a = p ? to_g2a(p) : pg::g2_generator();
    if (!g2a_is_reduced(a)) return fail(PG_ERR_INVALID_ARGUMENT, "coordinates not reduced");
    if (!pg::g2a_on_curve(a)) return fail(PG_ERR_INVALID_ARGUMENT, "the point is not on the twist");
    const pg::Fr canon = pg::fr_from_mont(to_fr(k));
    const pg::G2A r = pg::g2a_mul(a, canon.l);
    std::memcpy(out, &r, sizeof r);
    return PG_OK;
}

pg_status pg_g2_to_compressed(const pg_g2_affine *in, uint64_t count, uint8_t *out) {
    if (count && (!in || !out)) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t n = 0; n < count; n++) {
        const pg::G2A a = to_g2a(in + n);
        if (!g2a_is_reduced(a)) return fail(PG_ERR_INVALID_ARGUMENT, "coordinates not reduced");
        uint8_t *o = out + 96 * n;
        if (pg::g2a_is_identity(a)) {
            std::memset(o, 0, 96);
            o[0] = 0xc0;
            continue;
        }
        const pg::Fq x1 = pg::fq_from_mont(a.x.c1), x0 = pg::fq_from_mont(a.x.c0);
        for (int i = 0; i < 48; i++) {
            o[i] = (uint8_t)(x1.l[5 - i / 8] >> (8 * (7 - i % 8)));
            o[48 + i] = (uint8_t)(x0.l[5 - i / 8] >> (8 * (7 - i % 8)));
        }
        // y is the larger of (y, -y), compared by c1 first and then c0
        const pg::Fq2 ny = pg::fq2_neg(a.y);
        const pg::Fq ya[2] = {pg::fq_from_mont(a.y.c1), pg::fq_from_mont(a.y.c0)}, yb[2] = {pg::fq_from_mont(ny.c1), pg::fq_from_mont(ny.c0)};
        bool greater = false, decided = false;
        for (int h = 0; h < 2 && !decided; h++)
            for (int i = 5; i >= 0 && !decided; i--)
                if (ya[h].l[i] != yb[h].l[i]) {
                    greater = ya[h].l[i] > yb[h].l[i];
                    decided = true;
                }
        o[0] |= 0x80;
        if (greater) o[0] |= 0x20;
    }
    return PG_OK;
}

pg_status pg_g2_prepare(pg_engine *e, const pg_g2_affine *q, pg_g2_prepared **out) {
    if (!e || !q || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    const pg::G2A a = to_g2a(q);
    if (!g2a_is_reduced(a)) return fail(PG_ERR_INVALID_ARGUMENT, "coordinates not reduced");
    if (pg::g2a_is_identity(a)) return fail(PG_ERR_INVALID_ARGUMENT, "the identity cannot be prepared");
    if (!pg::g2a_on_curve(a)) return fail(PG_ERR_INVALID_ARGUMENT, "the point is not on the twist");
    std::vector<pg::G2Line> lines(pg::kAteLines);
    pg::g2_prepare(a, lines.data());
    PG_HIP_TRY(hipSetDevice(e->device));
    std::unique_ptr<pg_g2_prepared> p(new (std::nothrow) pg_g2_prepared);
    if (!p) return fail(PG_ERR_HIP, "out of host memory");
    p->device = e->device;
    const uint64_t bytes = lines.size() * sizeof(pg::G2Line);
    if (p->lines.reserve(bytes) != PG_OK) return fail(PG_ERR_HIP, std::string("pg_g2_prepare: ") + pg_last_error());
    const hipError_t err = hipMemcpy(p->lines.get(), lines.data(), bytes, hipMemcpyHostToDevice);
    if (err != hipSuccess) return fail(PG_ERR_HIP, std::string("pg_g2_prepare: ") + hipGetErrorString(err));
    *out = p.release();
    return PG_OK;
}

void pg_g2_prepared_destroy(pg_g2_prepared *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

pg_status pg_pairing_check(pg_engine *e, const pg_g1_affine *d_points, const pg_g2_prepared *const *prepared, uint64_t n_checks,
                           uint64_t n_pairs, uint8_t *d_ok, void *stream) {
    if (!d_ok) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return launch_pairing(e, d_points, prepared, n_checks, n_pairs, d_ok, nullptr, stream);
}

pg_status pg_pairing_gt(pg_engine *e, const pg_g1_affine *d_points, const pg_g2_prepared *const *prepared, uint64_t n_checks,
                        uint64_t n_pairs, uint64_t *d_gt, void *stream) {
    PG_TRY(check_scalars(d_gt, "d_gt"));
    return launch_pairing(e, d_points, prepared, n_checks, n_pairs, nullptr, d_gt, stream);
}

}  // extern "C"
