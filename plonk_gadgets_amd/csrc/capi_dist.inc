// capi_dist.inc -- the multi-GPU slice of the C ABI (included by capi.hip inside its translation unit).
//
// SURVEY.md section 8e / BASELINE.json config 5: witnesses are independent, so a batch shards over ranks as contiguous
// witness ranges that every rank emits at its GLOBAL numbering (pure arithmetic, no exchange); the one collective is
// the all-gather that gives every rank every shard's columns.  RCCL is bound at run time (dlsym/dlopen), never linked:
// a single-GPU user of the library needs no librccl at all, and inside a process that already carries an RCCL (a
// PyTorch host) the communicator is created by THAT copy of the library.
#include <dlfcn.h>

// RCCL's types, without requiring its development header (a single-GPU box need not have it): the handful this file uses,
// with the values of rccl.h (NCCL's ABI, stable since NCCL 2); checked against the real header where there is one.
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
static_assert(sizeof(ncclUniqueId) == 128 && ncclSuccess == 0 && ncclUint64 == 5, "RCCL ABI differs from the local declarations");
#else
#define NCCL_UNIQUE_ID_BYTES 128
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[NCCL_UNIQUE_ID_BYTES]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclUint8 = 1, ncclUint64 = 5 } ncclDataType_t;
#endif

struct pg_comm {
    pg_engine *e = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    bool owned = false;  // created by pg_comm_create (destroyed with it) or adopted from the host
    Scratch d_totals;  // 2 + 2 * world words: the staging buffer of the ragged plans' totals exchange
};

namespace {

struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string why;
};

RcclApi g_rccl;

template <class F>
bool bind_sym(void *h, const char *name, F &slot) {
    void *p = h ? dlsym(h, name) : dlsym(RTLD_DEFAULT, name);
    slot = reinterpret_cast<F>(p);
    return p != nullptr;
}

bool bind_all(void *h) {
    RcclApi a;
    a.handle = h;
    const bool ok = bind_sym(h, "ncclGetUniqueId", a.GetUniqueId) && bind_sym(h, "ncclCommInitRank", a.CommInitRank) &&
                    bind_sym(h, "ncclCommDestroy", a.CommDestroy) && bind_sym(h, "ncclCommCount", a.CommCount) &&
                    bind_sym(h, "ncclCommUserRank", a.CommUserRank) && bind_sym(h, "ncclAllGather", a.AllGather) &&
                    bind_sym(h, "ncclGroupStart", a.GroupStart) && bind_sym(h, "ncclGroupEnd", a.GroupEnd) &&
                    bind_sym(h, "ncclGetErrorString", a.GetErrorString);
    if (ok) {
        a.ok = true;
        g_rccl = a;
    }
    return ok;
}

// the process's RCCL: one that is already loaded (a PyTorch host brings its own) before any other
pg_status rccl() {
    if (g_rccl.ok) return PG_OK;
    if (const char *path = std::getenv("PG_RCCL_LIB")) {
        void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        const char *why = h ? nullptr : dlerror();  // (read once, at once: dlerror() clears itself, and bind_all's dlsym calls overwrite it)
        const std::string reason = why ? why : "symbols missing";
        if (h && bind_all(h)) return PG_OK;
        return fail(PG_ERR_HIP, std::string("PG_RCCL_LIB=") + path + " is not a usable RCCL: " + reason);
    }
    if (bind_all(nullptr)) return PG_OK;  // global scope
    const char *names[] = {"librccl.so", "librccl.so.1"};
    for (const char *n : names) {
        void *h = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
        if (h && bind_all(h)) return PG_OK;
    }
    const char *load[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : load) {
        void *h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (h && bind_all(h)) return PG_OK;
    }
    return fail(PG_ERR_HIP, "RCCL not found (looked in the process, then librccl.so.1 / librccl.so / /opt/rocm/lib; set PG_RCCL_LIB)");
}

#define PG_NCCL_TRY(expr)                                                                                   \
    do {                                                                                                    \
        ncclResult_t _r = (expr);                                                                           \
        if (_r != ncclSuccess) return fail(PG_ERR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(_r)); \
    } while (0)

// the handle of a communicator of `world` ranks, with its staging words on the engine's device; an owned communicator is
// destroyed with the handle, also when this fails
pg_status comm_handle(pg_engine *e, ncclComm_t comm, int rank, int world, bool owned, pg_comm **out) {
    std::unique_ptr<pg_comm, void (*)(pg_comm *)> c(new (std::nothrow) pg_comm(), pg_comm_destroy);
    if (!c) {
        if (owned) (void)g_rccl.CommDestroy(comm);
        return fail(PG_ERR_HIP, "out of host memory");
    }
    c->e = e;
    c->comm = comm;
    c->rank = rank;
    c->world = world;
    c->owned = owned;
    if (hipSetDevice(e->device) != hipSuccess || c->d_totals.reserve((2 + 2 * (size_t)world) * sizeof(uint64_t)) != PG_OK)
        return fail(PG_ERR_HIP, "hipMalloc(totals staging)");
    *out = c.release();
    return PG_OK;
}

inline uint64_t up2(uint64_t words) { return (words + 15) & ~15ull; }  // sections of a packed chunk start on 128-byte lines (the sweeps' wave stores do)

}  // namespace

extern "C" {

/* ---- shards ------------------------------------------------------------------- */
pg_status pg_shard_range(uint64_t total, uint32_t rank, uint32_t world, uint64_t *lo, uint64_t *hi) {
    if (!lo || !hi) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (world == 0 || rank >= world) return fail(PG_ERR_INVALID_ARGUMENT, "rank must be below world");
    const uint64_t base = total / world, rem = total % world;
    *lo = (uint64_t)rank * base + (rank < rem ? rank : rem);
    *hi = *lo + base + (rank < rem ? 1 : 0);
    return PG_OK;
}

pg_status pg_range_check_shard_layout(const pg_scalar *min_range, const pg_scalar *max_range, uint64_t total, uint32_t rank,
                                      uint32_t world, uint64_t gate_base, uint64_t var_base, pg_shard *out) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t lo, hi;
    PG_TRY(pg_shard_range(total, rank, world, &lo, &hi));
    pg_layout lay;
    PG_TRY(pg_range_check_layout(min_range, max_range, hi - lo, &lay));
    out->rank = rank;
    out->world = world;
    out->lo = lo;
    out->hi = hi;
    out->gate_base = gate_base + lo * lay.gates_per_item;
    out->var_base = var_base + lo * lay.vars_per_item;
    out->n_gates = lay.n_gates;
    out->n_vars = lay.n_vars;
    return PG_OK;
}

pg_status pg_range_check_sharded_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range,
                                       const pg_scalar *d_witness_local, uint64_t total, uint32_t rank, uint32_t world,
                                       uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                       pg_variable *d_result_vars, pg_shard *shard, void *stream) {
    pg_shard s;
    PG_TRY(pg_range_check_shard_layout(min_range, max_range, total, rank, world, gate_base, var_base, &s));
    if (shard) *shard = s;
    return pg_range_check_batch(e, min_range, max_range, d_witness_local, s.hi - s.lo, s.gate_base, s.var_base, out,
                                d_result_vars, stream);
}

/* ---- packed chunks: all nine arrays of a call back to back, one collective per chunk ----------- */
pg_status pg_packed_layout(uint64_t n_gates, uint64_t n_vars, pg_packed *out) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t cur = 0;
    for (int i = 0; i < 5; i++) { out->q_words[i] = cur; cur += up2(n_gates * 4); }
    for (int i = 0; i < 3; i++) { out->w_words[i] = cur; cur += up2(n_gates); }
    out->var_words = cur;
    cur += up2(n_vars * 4);
    out->total_words = cur;
    out->n_gates = n_gates;
    out->n_vars = n_vars;
    return PG_OK;
}

pg_status pg_columns_in_packed(void *d_packed, uint64_t n_gates, uint64_t n_vars, pg_columns *out) {
    if (!out || !d_packed || !aligned(d_packed, 16)) return fail(PG_ERR_INVALID_ARGUMENT, "packed buffer NULL or not 16-byte aligned");
    pg_packed p;
    PG_TRY(pg_packed_layout(n_gates, n_vars, &p));
    uint64_t *w = static_cast<uint64_t *>(d_packed);
    out->q_m = reinterpret_cast<pg_scalar *>(w + p.q_words[0]);
    out->q_l = reinterpret_cast<pg_scalar *>(w + p.q_words[1]);
    out->q_r = reinterpret_cast<pg_scalar *>(w + p.q_words[2]);
    out->q_o = reinterpret_cast<pg_scalar *>(w + p.q_words[3]);
    out->q_c = reinterpret_cast<pg_scalar *>(w + p.q_words[4]);
    out->w_l = w + p.w_words[0];
    out->w_r = w + p.w_words[1];
    out->w_o = w + p.w_words[2];
    out->var_values = reinterpret_cast<pg_scalar *>(w + p.var_words);
    return PG_OK;
}

/* ---- communicator ---------------------------------------------------------------- */
pg_status pg_comm_unique_id(uint8_t id[PG_COMM_ID_BYTES]) {
    if (!id) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(rccl());
    static_assert(PG_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "pg_comm id size");
    ncclUniqueId u;
    PG_NCCL_TRY(g_rccl.GetUniqueId(&u));
    std::memcpy(id, u.internal, PG_COMM_ID_BYTES);
    return PG_OK;
}

const char *pg_comm_library(void) {
    static std::string path;
    if (rccl() != PG_OK) return "";
    Dl_info info{};
    if (dladdr(reinterpret_cast<const void *>(g_rccl.AllGather), &info) && info.dli_fname) path = info.dli_fname;
    return path.c_str();
}

pg_status pg_comm_create(pg_engine *e, const uint8_t id[PG_COMM_ID_BYTES], uint32_t rank, uint32_t world, pg_comm **out) {
    if (!e || !id || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (world == 0 || rank >= world) return fail(PG_ERR_INVALID_ARGUMENT, "rank must be below world");
    PG_TRY(rccl());
    PG_HIP_TRY(hipSetDevice(e->device));
    ncclUniqueId u;
    std::memcpy(u.internal, id, PG_COMM_ID_BYTES);
    ncclComm_t comm = nullptr;
    PG_NCCL_TRY(g_rccl.CommInitRank(&comm, (int)world, u, (int)rank));
    return comm_handle(e, comm, (int)rank, (int)world, true, out);
}

pg_status pg_comm_adopt(pg_engine *e, void *nccl_comm, pg_comm **out) {
    if (!e || !nccl_comm || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    PG_TRY(rccl());
    int n = 0, r = 0;
    PG_NCCL_TRY(g_rccl.CommCount(static_cast<ncclComm_t>(nccl_comm), &n));
    PG_NCCL_TRY(g_rccl.CommUserRank(static_cast<ncclComm_t>(nccl_comm), &r));
    return comm_handle(e, static_cast<ncclComm_t>(nccl_comm), r, n, false, out);
}

// ordering only: the engine's device current, an owned communicator destroyed before its staging words go
void pg_comm_destroy(pg_comm *c) {
    if (!c) return;
    (void)hipSetDevice(c->e->device);
    if (c->owned && c->comm && g_rccl.ok) (void)g_rccl.CommDestroy(c->comm);
    delete c;
}

uint32_t pg_comm_rank(const pg_comm *c) { return c ? (uint32_t)c->rank : 0; }
uint32_t pg_comm_world(const pg_comm *c) { return c ? (uint32_t)c->world : 0; }

/* ---- collectives (enqueued on `stream`, ordered after whatever the stream holds) ---------- */
pg_status pg_allgather_bytes(pg_comm *c, const void *d_send, void *d_recv, uint64_t bytes_per_rank, void *stream) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "communicator is NULL");
    if (bytes_per_rank == 0) return PG_OK;
    if (!d_send || !d_recv) return fail(PG_ERR_INVALID_ARGUMENT, "buffer is NULL");
    if (bytes_per_rank & 7) return fail(PG_ERR_INVALID_ARGUMENT, "bytes_per_rank must be a multiple of 8");
    PG_HIP_TRY(hipSetDevice(c->e->device));
    PG_NCCL_TRY(g_rccl.AllGather(d_send, d_recv, bytes_per_rank / 8, ncclUint64, c->comm, static_cast<hipStream_t>(stream)));
    return PG_OK;
}

pg_status pg_allgather_columns(pg_comm *c, const pg_columns *local, uint64_t n_gates, uint64_t n_vars, const pg_columns *gathered,
                               void *stream) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "communicator is NULL");
    PG_TRY(check_columns(local));
    PG_TRY(check_columns(gathered));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const void *src[9] = {local->q_m, local->q_l, local->q_r, local->q_o, local->q_c, local->w_l, local->w_r, local->w_o, local->var_values};
    void *dst[9] = {gathered->q_m, gathered->q_l, gathered->q_r, gathered->q_o, gathered->q_c,
                    gathered->w_l, gathered->w_r, gathered->w_o, gathered->var_values};
    const uint64_t words[9] = {n_gates * 4, n_gates * 4, n_gates * 4, n_gates * 4, n_gates * 4, n_gates, n_gates, n_gates, n_vars * 4};
    // one group: RCCL fuses the nine gathers into one launch; rank order == witness order, so each gathered column is
    // the whole batch's column, contiguous
    PG_NCCL_TRY(g_rccl.GroupStart());
    ncclResult_t bad = ncclSuccess;
    for (int i = 0; i < 9; i++) {
        if (words[i] == 0) continue;
        ncclResult_t r = g_rccl.AllGather(src[i], dst[i], words[i], ncclUint64, c->comm, st);
        if (r != ncclSuccess && bad == ncclSuccess) bad = r;
    }
    ncclResult_t end = g_rccl.GroupEnd();
    if (bad != ncclSuccess) return fail(PG_ERR_HIP, std::string("ncclAllGather: ") + g_rccl.GetErrorString(bad));
    if (end != ncclSuccess) return fail(PG_ERR_HIP, std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(end));
    return PG_OK;
}


/* ---- the chunked gather pipeline (BASELINE config 5) ------------------------------------------------------------ */
}  // extern "C"

struct pg_gather_pipeline {
    pg_comm *c = nullptr;
    int device = 0;  // (kept here: the pipeline may outlive its communicator by the time it is destroyed)
    pg_scalar mn{}, mx{};
    uint64_t chunk = 0;
    bool vars_only = false;
    pg_layout lay{};
    pg_packed packed{};   // a rank's chunk: all nine arrays (packed mode) / the eight row arrays (variables-only mode)
    Stream comm_stream;
    Event ready[2], done[2];
    // packed mode: local[b] = this rank's chunk, gathered[b] = every rank's; variables-only: gathered[b] = every rank's rows
    // (regenerated here), own[b] = this rank's variable table, vars[b] = every rank's
    Scratch local[2], gathered[2], own[2], vars[2];  // (words: uint64_t)
    Scratch res;                                     // pg_variable per item of a chunk
    std::vector<pg_columns> parts[2];
    pg_columns mine[2];   // where this rank's emission of a slot goes
};

extern "C" {

// ordering only: the pipeline's device current, its communication stream drained.  The members release themselves.
void pg_range_check_gather_pipeline_destroy(pg_gather_pipeline *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->comm_stream.get());
    delete p;
}

pg_status pg_range_check_gather_pipeline_create(pg_comm *c, const pg_scalar *min_range, const pg_scalar *max_range, uint64_t chunk,
                                                uint32_t variables_only, pg_gather_pipeline **out) {
    if (!c || !min_range || !max_range || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (chunk == 0) return fail(PG_ERR_INVALID_ARGUMENT, "chunk must be positive");
    pg_layout lay;
    PG_TRY(pg_range_check_layout(min_range, max_range, chunk, &lay));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    // (nothing is enqueued here: on a failure the members release themselves, the device current)
    std::unique_ptr<pg_gather_pipeline> p(new (std::nothrow) pg_gather_pipeline());
    if (!p) return fail(PG_ERR_HIP, "out of host memory");
    p->c = c;
    p->device = c->e->device;
    p->mn = *min_range;
    p->mx = *max_range;
    p->chunk = chunk;
    p->vars_only = variables_only != 0;
    p->lay = lay;
    const uint64_t world = (uint64_t)c->world, G = lay.n_gates, V = lay.n_vars;
    pg_status st = pg_packed_layout(G, p->vars_only ? 0 : V, &p->packed);
    if (st != PG_OK) return fail(st, "packed layout");
    const uint64_t words = p->packed.total_words;
    if (p->comm_stream.create(hipStreamNonBlocking) != PG_OK) return fail(PG_ERR_HIP, "communication stream");
    if (p->res.reserve(chunk * sizeof(pg_variable)) != PG_OK) return fail(PG_ERR_HIP, "hipMalloc");
    for (int b = 0; b < 2; b++) {
        if (p->ready[b].create(hipEventDisableTiming) != PG_OK || p->done[b].create(hipEventDisableTiming) != PG_OK)
            return fail(PG_ERR_HIP, "events");
        if (p->gathered[b].reserve(world * words * 8) != PG_OK) return fail(PG_ERR_HIP, "hipMalloc(gathered chunk)");
        if (p->vars_only) {
            if (p->own[b].reserve(V * 32) != PG_OK || p->vars[b].reserve(world * V * 32) != PG_OK)
                return fail(PG_ERR_HIP, "hipMalloc(variable tables)");
        } else if (p->local[b].reserve(words * 8) != PG_OK) {
            return fail(PG_ERR_HIP, "hipMalloc(local chunk)");
        }
        p->parts[b].resize(world);
        for (uint64_t r = 0; r < world; r++) {
            pg_columns &pc = p->parts[b][r];
            if ((st = pg_columns_in_packed(p->gathered[b].as<uint64_t>() + r * words, G, p->vars_only ? 0 : V, &pc)) != PG_OK)
                return fail(st, "packed view");
            if (p->vars_only) pc.var_values = reinterpret_cast<pg_scalar *>(p->vars[b].as<uint64_t>() + r * V * 4);
        }
        if (p->vars_only) {  // own rows straight into their place among everybody's, own variables into the send buffer
            p->mine[b] = p->parts[b][(uint64_t)c->rank];
            p->mine[b].var_values = p->own[b].as<pg_scalar>();
        } else if ((st = pg_columns_in_packed(p->local[b].get(), G, V, &p->mine[b])) != PG_OK) {
            return fail(st, "packed view");
        }
    }
    *out = p.release();
    return PG_OK;
}

uint64_t pg_range_check_gather_pipeline_bytes_per_chunk(const pg_gather_pipeline *p) {
    if (!p) return 0;
    return p->vars_only ? p->lay.n_vars * 32 : p->packed.total_words * 8;
}

pg_status pg_range_check_gather_pipeline_run(pg_gather_pipeline *p, const pg_scalar *d_witness_local, uint64_t total_per_rank,
                                             uint64_t gate_base, uint64_t var_base, pg_chunk_consumer consume, void *user,
                                             void *stream) {
    if (!p || (!d_witness_local && total_per_rank)) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (total_per_rank % p->chunk) return fail(PG_ERR_INVALID_ARGUMENT, "total_per_rank must be a multiple of the pipeline's chunk");
    pg_comm *c = p->c;
    pg_engine *e = c->e;
    PG_HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t G = p->lay.gates_per_item, V = p->lay.vars_per_item, world = (uint64_t)c->world, rank = (uint64_t)c->rank;
    const uint64_t nchunks = total_per_rank / p->chunk;
    int pending_slot = -1;
    uint64_t pending_chunk = 0;
    auto finish = [&]() -> pg_status {  // the chunk on the links is complete for `st`; hand it over
        if (pending_slot < 0) return PG_OK;
        PG_HIP_TRY(hipStreamWaitEvent(st, p->done[pending_slot].get(), 0));
        if (consume) consume(user, pending_chunk, (uint32_t)world, p->parts[pending_slot].data(), p->lay.n_gates, p->lay.n_vars, stream);
        pending_slot = -1;
        return PG_OK;
    };
    for (uint64_t k = 0; k < nchunks; k++) {
        const int b = (int)(k & 1);
        // emission of chunk k into slot b on the caller's stream: behind the consumer of chunk k - 2 (same stream), which
        // had been made to wait for that chunk's collective
        for (uint64_t r = 0; r < (p->vars_only ? world : 1); r++) {
            const uint64_t who = p->vars_only ? r : rank, first = who * total_per_rank + k * p->chunk;
            if (who == rank) {
                PG_TRY(pg_range_check_batch(e, &p->mn, &p->mx, d_witness_local + k * p->chunk, p->chunk, gate_base + first * G,
                                            var_base + first * V, &p->mine[b], p->res.as<pg_variable>(), stream));
            } else {
                PG_TRY(pg_range_check_structure_batch(e, &p->mn, &p->mx, p->chunk, gate_base + first * G, var_base + first * V,
                                                      &p->parts[b][r], stream));
            }
        }
        PG_TRY(finish());  // chunk k - 1 (it travelled while chunk k was being emitted)
        // the collective of chunk k on the communication stream, behind the emission and behind everything the consumers
        // of earlier chunks have enqueued (they may still be reading the slot's gathered buffer)
        PG_HIP_TRY(hipEventRecord(p->ready[b].get(), st));
        PG_HIP_TRY(hipStreamWaitEvent(p->comm_stream.get(), p->ready[b].get(), 0));
        if (p->vars_only) PG_TRY(pg_allgather_bytes(c, p->own[b].get(), p->vars[b].get(), p->lay.n_vars * 32, p->comm_stream.get()));
        else PG_TRY(pg_allgather_bytes(c, p->local[b].get(), p->gathered[b].get(), p->packed.total_words * 8, p->comm_stream.get()));
        PG_HIP_TRY(hipEventRecord(p->done[b].get(), p->comm_stream.get()));
        pending_slot = b;
        pending_chunk = k;
    }
    return finish();
}

/* ---- ragged sharded batches: plan, exchange the totals, emit at the global numbering --------------------------------- */
pg_status pg_max_bound_ragged_sharded_plan(pg_comm *c, const pg_scalar *d_max_range_local, uint64_t batch_local, uint32_t *d_num_bits,
                                           uint64_t *d_row_off, uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base,
                                           pg_shard *shard, uint64_t *gates_per_rank, uint64_t *vars_per_rank, void *stream) {
    if (!c || !shard) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    pg_engine *e = c->e;
    pg_layout lay{};
    // a rank whose own plan fails still takes part in the exchange (the others would wait in it for ever) and sends a
    // sentinel: every rank then returns an error
    const pg_status planned = pg_max_bound_ragged_plan(e, d_max_range_local, batch_local, d_num_bits, d_row_off, d_var_off, &lay, stream);
    const std::string plan_error = planned == PG_OK ? std::string() : std::string(pg_last_error());
    const uint64_t world = (uint64_t)c->world, kFailed = ~0ull;
    std::vector<uint64_t> all(2 * world, 0);
    if (world == 1) {
        if (planned != PG_OK) return planned;
        all[0] = lay.n_gates;
        all[1] = lay.n_vars;
    } else {  // 16 bytes per rank through the collective, staged in the communicator's device words
        PG_HIP_TRY(hipSetDevice(e->device));
        uint64_t *d = c->d_totals.as<uint64_t>();
        const uint64_t mine[2] = {planned == PG_OK ? lay.n_gates : kFailed, planned == PG_OK ? lay.n_vars : kFailed};
        hipStream_t st = static_cast<hipStream_t>(stream);
        // (from here on nothing returns before the collective has been enqueued)
        const bool staged = hipMemcpyAsync(d, mine, sizeof mine, hipMemcpyHostToDevice, st) == hipSuccess;
        if (!staged) (void)hipMemsetAsync(d, 0xff, sizeof mine, st);
        pg_status s = pg_allgather_bytes(c, d, d + 2, sizeof mine, stream);
        if (s == PG_OK && (hipMemcpyAsync(all.data(), d + 2, 2 * world * sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
                           hipStreamSynchronize(st) != hipSuccess))
            s = fail(PG_ERR_HIP, "reading the gathered totals back");
        if (s != PG_OK) return s;
        if (planned != PG_OK) return fail(planned, plan_error);
        if (!staged) return fail(PG_ERR_HIP, "hipMemcpyAsync(totals)");
        for (uint64_t r = 0; r < world; r++)
            if (all[2 * r] == kFailed) return fail(PG_ERR_HIP, "the plan of rank " + std::to_string(r) + " failed: nothing emitted on any rank");
    }
    uint64_t g0 = gate_base, v0 = var_base;
    for (uint64_t r = 0; r < world; r++) {
        if (r < (uint64_t)c->rank) { g0 += all[2 * r]; v0 += all[2 * r + 1]; }
        if (gates_per_rank) gates_per_rank[r] = all[2 * r];
        if (vars_per_rank) vars_per_rank[r] = all[2 * r + 1];
    }
    shard->rank = (uint32_t)c->rank;
    shard->world = (uint32_t)c->world;
    shard->lo = shard->hi = 0;  // (witness positions are the host's: a ragged batch is sharded by its caller)
    shard->gate_base = g0;
    shard->var_base = v0;
    shard->n_gates = lay.n_gates;
    shard->n_vars = lay.n_vars;
    return PG_OK;
}

pg_status pg_max_bound_ragged_sharded_batch(pg_comm *c, const pg_scalar *d_max_range_local, const pg_scalar *d_witness_local,
                                            uint64_t batch_local, uint32_t *d_num_bits, uint64_t *d_row_off, uint64_t *d_var_off,
                                            uint64_t gate_base, uint64_t var_base, const pg_columns *out, pg_variable *d_result_vars,
                                            pg_shard *shard, void *stream) {
    pg_shard s;
    PG_TRY(pg_max_bound_ragged_sharded_plan(c, d_max_range_local, batch_local, d_num_bits, d_row_off, d_var_off, gate_base, var_base,
                                            &s, nullptr, nullptr, stream));
    if (shard) *shard = s;
    return pg_max_bound_ragged_batch(c->e, d_max_range_local, d_witness_local, batch_local, d_num_bits, d_row_off, d_var_off,
                                     s.gate_base, s.var_base, out, d_result_vars, stream);
}
}  // extern "C"
