// capi_composer.inc -- pg_composer (included by capi.hip inside its translation unit).

// device arrays a ragged call plans into and, once its rows are emitted, the composer keeps for its footprint (words: uint64_t;
// num_bits: uint32_t, calls with per-item bounds only)
struct RaggedBuffers {
    Scratch row_off, var_off, num_bits;
    uint64_t *rows() const { return row_off.as<uint64_t>(); }
    uint64_t *vars() const { return var_off.as<uint64_t>(); }
    uint32_t *bits() const { return num_bits.as<uint32_t>(); }
};

// Everything the composer owns is a member that releases itself (owners.hpp): pg_composer_destroy makes the engine's device
// current, drains the stream and deletes.  After that no member depends on another, so their order says nothing about release.
struct pg_composer {
    pg_engine *e = nullptr;
    hipStream_t stream = nullptr;
    uint64_t n = 0, nvars = 0, zero_var = 0;
    // the nine columns: separate arrays, or ONE block with the selector columns a stride apart (pg_composer_spread_columns)
    ColumnStore cols;
    Scratch d_stage;  // a StageBlob: inputs of single-gadget calls
    uint64_t *stage_words() const { return d_stage.as<uint64_t>(); }
    Scratch d_preflight;  // a pg::Preflight: what the passes over an append's device arrays leave (preflight())
    // public_inputs_sparse_store and the rows with a live fourth wire (host copies; uploaded by check/materialize)
    std::vector<uint64_t> pi_gate;
    std::vector<pg_scalar> pi_val;
    std::vector<pg::FourthWire> fourth;
    // the rows of the range widget (range_gate.hpp): where q_range = 1 (host list; written by materialize, checked by check)
    std::vector<pg::RangeSeg> range_segs;
    // footprints of the batched calls (permutation.hpp) and the grow-only scratch of pg_composer_permutation
    std::vector<pg::PermSeg> segs;
    Scratch perm_small, perm_big, val_ws;  // val_ws: gathered assignments of batched calls
    Scratch perm_pieces;  // pg_composer_permutation: the first item of every piece of a ragged ladder segment's rows
    Scratch wsum_ws;  // pg_composer_weighted_sum_ragged_batch: its tiles' aggregates and carries (weighted_sum.hpp)
    std::vector<RaggedBuffers> ragged;  // device prefix sums / ladder lengths of the ragged calls (referenced by segs)
    Pinned h_total;  // 64 bytes: what a call reads back, a preflight its pg::Preflight (made by pg_composer_create)
    uint64_t *totals() const { return h_total.as<uint64_t>(); }
    uint64_t perm_last_sparse = 0;  // size of the sparse list the last permutation needed
    uint64_t sparse_hint = 0;       // wire positions the batched calls so far are expected to put on that list
    uint64_t sparse_cap_first = 0;  // pg_composer_permutation_reserve: first-pass size of that list (0: estimate)
    bool auto_grow = false;
    // ---- the command queue (single composer calls are recorded on the host and flushed as few launches) ----
    struct Queued {
        uint8_t kind;        // 0: a gate call (g); 1: range_check; 2: max_bound -- on an allocated witness
        pg::GateCmd g;       // kind 0
        pg::Fr b0, b1;       // kind 1: min_range, max_range; kind 2: max_range in b1
        uint32_t num_bits;   // ladder length of the gadget call
        uint64_t wvar;       // the witness Variable
        pg::Fr wval;         // and its assignment (AllocatedScalar.scalar)
        uint64_t gate, var;  // first row / first Variable the call was given
        bool in_place = false;  // a witness refresh: the call's rows are already in the columns
    };
    std::vector<Queued> queue;
    bool queueing = true;
    // the layout of the last single range_check / max_bound (the ladder length is ~500 host field operations: a loop of
    // single calls with the same public bounds should pay them once)
    pg_scalar last_min{}, last_max{};
    pg_layout last_lay{};
    int last_kind = 0;  // 0: none, 1: range_check, 2: max_bound
    // staging of a flush: pinned host memory and its device twin (grow-only), carved up run by run, so that the uploads
    // are truly asynchronous.  TWO such pairs take turns: a flush waits for the flush before the last one (the event recorded
    // at its end) before refilling that pair, not for the one the device may still be working on.
    Staging staging[2];
    int stage = 0;  // the pair the current flush fills
    size_t queue_used = 0;
    uint64_t flushes = 0, flush_launches = 0;  // statistics (pg_composer_queue_stats)
    // ---- witness refresh (pg_composer_clear_witness) ------------------------------------------------------------------
    // Every append whose ROWS are a function of host-visible things alone -- the call, its public parameters and where it
    // lands (first row, first Variable, zero_var) -- leaves a signature of exactly those things, in order.  After
    // clear_witness the same calls come again with other witnesses: while every such append matches the signature the
    // previous build left at the same place in the sequence, its rows are already in the columns (nothing has written there
    // since: appends only ever write at and beyond the composer's end) and only its assignments are written.  The first
    // append that differs ends it: the rest of the old log is dropped and everything is emitted in full again.  Appends
    // whose rows depend on device arrays leave no signature and are always emitted in full (which is always right).
    struct Sig {
        uint64_t a, b;
        bool operator==(const Sig &o) const { return a == o.a && b == o.b; }
    };
    std::vector<Sig> log;
    size_t cursor = 0;  // refill: the entry of the previous build the next signed append is compared with
    bool refill = false;
    uint64_t n0 = 0, nvars0 = 0, old_n = 0;  // what pg_composer_create leaves; rows of the previous build (grow keeps them)
    size_t log0 = 0, fourth0 = 0;
    uint64_t rows_in_place = 0, rows_rewritten = 0;  // since the last clear_witness (pg_composer_refresh_stats)
    uint64_t unmatched = 0;  // makes the signature of every batch with failing items unique (their shape depends on witness values)
};

namespace {

pg_status flush(pg_composer *c);  // the command queue (below)

// two independent 64-bit FNV-1a style hashes over what an append's rows are a function of
struct SigHasher {
    uint64_t a = 0xcbf29ce484222325ull, b = 0x9e3779b97f4a7c15ull;
    void bytes(const void *p, size_t n) {
        const unsigned char *c = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; i++) {
            a = (a ^ c[i]) * 0x100000001b3ull;
            b = (b ^ c[i]) * 0xff51afd7ed558ccdull;
            b ^= b >> 29;
        }
    }
    void u64(uint64_t v) { bytes(&v, 8); }
    void fr(const pg::Fr &f) { bytes(f.l, 32); }
    pg_composer::Sig done() const { return pg_composer::Sig{a, b}; }
};
// The append that is about to write `rows` rows at the composer's end has signature s: are those rows in the columns
// already?  The DECISION (in_place) is a read-only comparison with the previous build's log.  The log itself is touched only
// by commit(), which an append calls once everything it launches has been enqueued: an append that fails after the decision
// (a NULL or misaligned array found by the engine call, a HIP error) leaves through the destructor, which ends a refresh
// at this place -- the rest of the old log is dropped, so nothing later is taken for "in place" on the strength of an entry whose
// rows this failed call may have overwritten in part -- and leaves no signature for rows that were never written (a
// different append at this row, then clear_witness, then the first call again must not find "its" rows there).
// `active` = false: an append that leaves no signature (an empty batch, add_input).
struct SignedAppend {
    pg_composer *c;
    pg_composer::Sig s;
    uint64_t rows;
    bool active, in_place, settled = false;
    SignedAppend(pg_composer *c_, const pg_composer::Sig &s_, uint64_t rows_, bool active_ = true)
        : c(c_), s(s_), rows(rows_), active(active_),
          in_place(active_ && c_->refill && c_->cursor < c_->log.size() && c_->log[c_->cursor] == s_) {}
    SignedAppend(const SignedAppend &) = delete;
    SignedAppend &operator=(const SignedAppend &) = delete;
    void end_refresh() {  // another circuit from here on
        if (c->refill) {
            c->refill = false;
            c->log.resize(c->cursor);
        }
    }
    void commit() {
        settled = true;
        if (!active) return;
        if (in_place) {
            c->cursor++;
            c->rows_in_place += rows;
            return;
        }
        end_refresh();
        c->log.push_back(s);
        c->rows_rewritten += rows;
    }
    ~SignedAppend() {
        if (!settled && active) end_refresh();
    }
};
// Which call an append's signature is for: the first word that gadget_sig and gate_batch hash.  Two calls never share one: a different
// append at the same place must not be taken for rows already in place, whatever its other words are.
// run_gate's signature (a single gate call) starts with cmd.op instead -- OP_ADD_INPUT .. OP_MUL = 0 .. 3 (composer.hpp), which
// RANGE_CHECK and MAX_BOUND meet in value.  That is no shared kind: run_gate hashes 240 bytes (six words, six scalars) where gadget_sig
// hashes 128 and gate_batch 232, and strings of different lengths agree only where the 128-bit hash itself collides -- the chance any
// two different appends take.
enum class SigKind : uint64_t {
    RANGE_CHECK = 1,                 // pg_range_check (= Queued::kind)
    MAX_BOUND = 2,                   // pg_max_bound (= Queued::kind)
    RANGE_CHECK_BATCH = 11,          // pg_composer_range_check_batch
    MAX_BOUND_BATCH = 12,            // pg_composer_max_bound_batch
    SCALAR_MIX_BATCH = 13,           // pg_composer_scalar_mix_batch
    RANGE_CHECK_ALLOCATED_BATCH = 21,  // pg_composer_range_check_allocated_batch
    MAX_BOUND_ALLOCATED_BATCH = 22,  // pg_composer_max_bound_allocated_batch
    DECOMPOSITION_BATCH = 23,        // pg_composer_scalar_decomposition_batch
    SELECT_ZERO_BATCH = 24,          // pg_composer_conditionally_select_zero_batch
    SELECT_ONE_BATCH = 25,           // pg_composer_conditionally_select_one_batch
    MAYBE_EQUAL_BATCH = 26,          // pg_composer_maybe_equal_batch
    RANGE_GATE_BATCH = 27,           // pg_composer_range_gate_batch, pg_composer_range_gate (a batch of one)
    IS_NON_ZERO_BATCH = 28,          // pg_composer_is_non_zero_batch
    GATE_BATCH = 29,                 // the gate batches (gate_batch: poly_gate, add, mul, constrain_to_constant, boolean_gate)
    RANGE_CHECK_RAGGED_BATCH = 30,   // pg_composer_range_check_ragged_batch
    MAX_BOUND_RAGGED_BATCH = 31,     // pg_composer_max_bound_ragged_batch (it signed with 27, range_gate's, until the kinds had names)
    DECOMPOSITION = 43,              // pg_scalar_decomposition_gadget
    INTERVAL_GATE_BATCH = 61,        // pg_composer_interval_gate_batch, pg_composer_interval_gate (a batch of one)
    INTERVAL_GATE_RAGGED_BATCH = 62,  // pg_composer_interval_gate_ragged_batch
    WEIGHTED_SUM_RAGGED_BATCH = 63,   // pg_composer_weighted_sum_ragged_batch
    IS_LESS_EQUAL_BATCH = 64          // pg_composer_is_less_equal_batch, pg_composer_is_less_equal (a batch of one)
};
// kind: which call; b0, b1: its public scalars; extra: a public integer; dg: the digest of the device arrays its rows depend on
pg_composer::Sig gadget_sig(const pg_composer *c, SigKind kind, const pg::Fr &b0, const pg::Fr &b1, uint64_t batch, uint64_t extra,
                            const pg_composer::Sig &dg = pg_composer::Sig{0, 0}) {
    SigHasher h;
    h.u64((uint64_t)kind); h.fr(b0); h.fr(b1); h.u64(batch); h.u64(extra); h.u64(dg.a); h.u64(dg.b);
    h.u64(c->n); h.u64(c->nvars); h.u64(c->zero_var);
    return h.done();
}

// new arrays for the live columns in the layout `stride` asks for (ColumnStore::grow: the composer is untouched when it fails)
pg_status grow(pg_composer *c, uint64_t gate_cap, uint64_t var_cap, uint64_t stride) {
    if (stride == c->cols.stride() && gate_cap <= c->cols.gate_cap() && var_cap <= c->cols.var_cap()) return PG_OK;
    PG_HIP_TRY(hipSetDevice(c->e->device));
    PG_TRY(flush(c));  // queued calls land in the buffers they were recorded against
    // (a witness refresh under way: the rows of the previous build beyond the composer's end are still wanted)
    const uint64_t cap = c->cols.gate_cap(), live_rows = c->refill && c->old_n > c->n ? (c->old_n < cap ? c->old_n : cap) : c->n;
    return c->cols.grow(gate_cap, var_cap, stride, live_rows, c->nvars, c->stream);
}
pg_status grow(pg_composer *c, uint64_t gate_cap, uint64_t var_cap) { return grow(c, gate_cap, var_cap, c->cols.stride()); }

pg_status need(pg_composer *c, uint64_t rows, uint64_t vars) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    if (c->n + rows > c->cols.gate_cap() || c->nvars + vars > c->cols.var_cap()) {
        if (c->auto_grow) {
            uint64_t g = c->cols.gate_cap(), v = c->cols.var_cap();
            if (c->n + rows > g) g = c->n + rows > 2 * g ? c->n + rows : 2 * g;
            if (c->nvars + vars > v) v = c->nvars + vars > 2 * v ? c->nvars + vars : 2 * v;
            return grow(c, g, v);
        }
        return fail(PG_ERR_CAPACITY, "composer capacity exceeded: " + std::to_string(c->n + rows) + " rows / " +
                                         std::to_string(c->nvars + vars) + " variables needed");
    }
    return PG_OK;
}

pg_status check_var(const pg_composer *c, pg_variable v) {
    // the reference indexes its HashMap and panics on an unknown Variable
    if (v >= c->nvars) return fail(PG_ERR_INVALID_ARGUMENT, "unknown Variable " + std::to_string(v));
    return PG_OK;
}

// The preflight of an append on device arrays, in ONE host synchronisation.  The composer's result block (digest.hpp) is cleared on
// its stream -- zeros, but the first `firsts` words of `call` ~0: the call's first offenders --, enqueue(block) launches the call's
// passes over its arrays, and the block comes back as r.  Every entry of the Variable arrays must be a Variable of this composer
// (the reference panics on an unknown one): that comes before the call's own preconditions, which the caller reads from r.call.
// Nothing has been appended when it fails.
template <class Enqueue>
pg_status preflight(pg_composer *c, unsigned firsts, pg::Preflight &r, Enqueue enqueue) {
    PG_HIP_TRY(hipSetDevice(c->e->device));
    pg::Preflight *d = c->d_preflight.as<pg::Preflight>();
    PG_HIP_TRY(hipMemsetAsync(d, 0, sizeof *d, c->stream));
    if (firsts) PG_HIP_TRY(hipMemsetAsync(d->call, 0xff, firsts * sizeof d->call[0], c->stream));
    enqueue(d);
    PG_HIP_TRY(hipGetLastError());
    PG_HIP_TRY(hipMemcpyAsync(c->totals(), d, sizeof *d, hipMemcpyDeviceToHost, c->stream));
    PG_HIP_TRY(hipStreamSynchronize(c->stream));
    r = *c->h_total.as<pg::Preflight>();
    if (r.max_var < c->nvars) return PG_OK;
    return fail(PG_ERR_INVALID_ARGUMENT, "unknown Variable " + std::to_string(r.max_var) + " in a batched append (the composer has " +
                                             std::to_string(c->nvars) + ")");
}
pg_composer::Sig sig_of(const pg::Digest &d) { return pg_composer::Sig{d.h1, d.h2}; }
// a preflight's pass over n words of a device array: their maximum into *max, and into *dg what they add to a digest under `salt`
void digest_words(pg_composer *c, const void *a, uint64_t n, unsigned long long *max, pg::Digest *dg, unsigned long long salt) {
    hipLaunchKernelGGL(pg::max_variable_kernel, dim3(grid_cap((n + pg::kThreads - 1) / pg::kThreads, (uint64_t)c->e->num_cus * 8)),
                       dim3(pg::kThreads), 0, c->stream, static_cast<const uint64_t *>(a), n, max, dg, salt);
}
// ... over the call's place-th array of Variables (NULL: the place is kept, nothing is read)
void digest_vars(pg_composer *c, const pg_variable *a, uint64_t n, pg::Preflight *d, unsigned place) {
    if (a) digest_words(c, a, n, &d->max_var, &d->vars, pg::var_array_salt(place));
}
// device arrays of Variables handed to a batched append: the preflight of the calls with no other device array.  `digest`: 128 bits
// over values and positions, the arrays salted by their place in the list -- what an append's rows depend on when its wires come
// from device memory (for its signature).
pg_status check_var_arrays(pg_composer *c, std::initializer_list<const pg_variable *> arrays, uint64_t batch,
                           pg_composer::Sig *digest = nullptr) {
    if (digest) *digest = pg_composer::Sig{0, 0};
    if (batch == 0) return PG_OK;
    pg::Preflight r;
    PG_TRY(preflight(c, 0, r, [&](pg::Preflight *d) {
        unsigned place = 0;
        for (const pg_variable *a : arrays) digest_vars(c, a, batch, d, place++);
    }));
    if (digest) *digest = sig_of(r.vars);
    return PG_OK;
}
// the preflight of the ragged ladders: the digest of their device arrays of per-item public bounds, n > 0 scalars each (the caller has
// returned on an empty batch; d2 may be NULL; the two arrays swapped digest differently).  No Variable comes from outside: max_var
// stays 0, which every composer knows (zero_var), and the words' maximum goes to call[0], which these calls do not read.
pg_status bounds_digest(pg_composer *c, const pg_scalar *d1, const pg_scalar *d2, uint64_t n, pg_composer::Sig *digest) {
    pg::Preflight r;
    PG_TRY(preflight(c, 0, r, [&](pg::Preflight *d) {
        digest_words(c, d1, 4 * n, &d->call[0], &d->others, pg::scalar_array_salt(0));
        if (d2) digest_words(c, d2, 4 * n, &d->call[0], &d->others, pg::scalar_array_salt(1));
    }));
    *digest = sig_of(r.others);
    return PG_OK;
}

pg_columns cols_at(const pg_composer *c, uint64_t gate, uint64_t var) {
    const pg::ComposerCols &v = c->cols.view();
    pg_columns o;
    o.q_m = reinterpret_cast<pg_scalar *>(v.q[0]) + gate;
    o.q_l = reinterpret_cast<pg_scalar *>(v.q[1]) + gate;
    o.q_r = reinterpret_cast<pg_scalar *>(v.q[2]) + gate;
    o.q_o = reinterpret_cast<pg_scalar *>(v.q[3]) + gate;
    o.q_c = reinterpret_cast<pg_scalar *>(v.q[4]) + gate;
    o.w_l = v.w[0] + gate;
    o.w_r = v.w[1] + gate;
    o.w_o = v.w[2] + gate;
    o.var_values = reinterpret_cast<pg_scalar *>(v.vars) + var;
    return o;
}

#ifndef PG_QUEUE_MAX
#define PG_QUEUE_MAX 8192  // entries; a full queue flushes itself
#endif

// room for one flush of n entries in the next staging pair; waits until the flush that last used it has left the device
pg_status queue_begin(pg_composer *c, size_t n) {
    const size_t bytes = n * sizeof(pg::GateCmd) + (n + 8) * 64;  // every entry at most one GateCmd, plus alignment slack per run
    c->stage ^= 1;
    Staging &S = c->staging[c->stage];
    if (bytes > S.size()) {  // both pairs grow together: the allocations (a millisecond each) fall into ONE flush
        const size_t want = bytes < (1u << 20) ? (1u << 20) : bytes * 2;
        PG_TRY(c->staging[c->stage ^ 1].acquire(want, true));
        PG_TRY(S.acquire(want, true));
    } else {
        PG_TRY(S.acquire(0, true));
    }
    c->queue_used = 0;
    return PG_OK;
}
// the next `bytes` of the staging pair (64-byte aligned): *h to fill, *d for the kernel
void queue_slice(pg_composer *c, size_t bytes, char **h, char **d) {
    const Staging &S = c->staging[c->stage];
    c->queue_used = (c->queue_used + 63) & ~(size_t)63;
    *h = S.host() + c->queue_used;
    *d = S.device() + c->queue_used;
    c->queue_used += bytes;
}

// gate calls of the queue, by index (ascending): <= kQueueRun commands per launch, levels computed per launch.  The entries are either
// consecutive (a run of gate calls) or rows-only gates picked from between the gadget calls of a loop (flush: they create no Variable)
pg_status flush_gate_list(pg_composer *c, const std::vector<size_t> &at) {
    std::vector<uint32_t> level_of;  // of the Variables this launch creates, by creation order
    size_t i = 0;
    const size_t j = at.size();
    while (i < j) {
        const size_t n = j - i < pg::kQueueRun ? j - i : pg::kQueueRun;
        char *h, *d;
        queue_slice(c, n * sizeof(pg::GateCmd), &h, &d);
        pg::GateCmd *cmds = reinterpret_cast<pg::GateCmd *>(h);
        level_of.clear();
        uint64_t first_var = c->nvars;  // no operand can reach it unless this launch creates Variables
        bool have_first = false;
        uint32_t max_level = 0;
        for (size_t k = 0; k < n; k++) {
            pg::GateCmd g = c->queue[at[i + k]].g;
            const bool creates = g.op != pg::OP_ROW;
            if (creates && !have_first) { first_var = g.var; have_first = true; }
            uint32_t lvl = 0;
            if (g.op == pg::OP_ADD || g.op == pg::OP_MUL) {
                auto lv = [&](uint64_t v) -> uint32_t {
                    return have_first && v >= first_var && v - first_var < level_of.size() ? level_of[v - first_var] : 0u;
                };
                const uint32_t la = lv(g.a), lb = lv(g.b);
                lvl = 1 + (la > lb ? la : lb);
                if (lvl > max_level) max_level = lvl;
            }
            g.pad = lvl;
            if (creates) level_of.push_back(lvl);
            if (c->queue[at[i + k]].in_place) g.op |= pg::OP_ROW_IN_PLACE;
            cmds[k] = g;
        }
        PG_HIP_TRY(hipMemcpyAsync(d, h, n * sizeof(pg::GateCmd), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(pg::gate_queue_kernel, dim3(1), dim3(1024), 0, c->stream, reinterpret_cast<const pg::GateCmd *>(d), (uint32_t)n,
                           first_var, max_level, c->cols.view());
        PG_HIP_TRY(hipGetLastError());
        c->flush_launches++;
        i += n;
    }
    return PG_OK;
}
// a run of gate calls [i, j) of the queue
pg_status flush_gates(pg_composer *c, size_t i, size_t j) {
    std::vector<size_t> at(j - i);
    for (size_t k = 0; k < at.size(); k++) at[k] = i + k;
    return flush_gate_list(c, at);
}

// The footprint joins the last one where it continues it in every respect (calls of one kind one after the other; a loop of single
// calls, flushed run by run), else it is one of its own.  only_if_long -- a run of queued single calls that went out as one batched
// launch: the same rows as the batched append of that gadget (a circuit built the reference's way, one allocate + range_check at a
// time: sigma of 17 M rows 3.5 -> 0.3 ms), but short runs stay what they were (rows of single calls): a footprint per run of two
// calls would be a launch per run in sigma.
// the ladder kinds whose batched append takes its public bounds per item (ragged_batch: the footprint keeps the call's prefix sums)
constexpr bool per_item_bounds_kind(uint32_t wire_kind) { return wire_kind == pg::WIRES_MAX_BOUND || wire_kind == pg::WIRES_RANGE_CHECK; }

void add_footprint(pg_composer *c, const pg::PermSeg &f, bool only_if_long = false) {
    if (!f.items) return;
    // what lets perm_route's questions be asked in any order (footprint.hpp)
    assert(!pg::is_template_kind(f.wire_kind) || f.wire_n == 0);
    // (the ladder kinds with a bound -- or a pair of bounds -- per item: never with a tail, never with a ladder length of the call's)
    assert(!f.row_off || f.wire_kind == pg::WIRES_UNKNOWN || pg::is_template_kind(f.wire_kind) ||
           (per_item_bounds_kind(f.wire_kind) && f.tail == 0 && f.wire_n == 0));
    pg::PermSeg *last = c->segs.empty() ? nullptr : &c->segs.back();
    if (last && !last->row_off && !f.row_off && last->gate_end == f.gate_base && last->var_end == f.var_base && last->L == f.L && last->V == f.V &&
        last->wire_kind == f.wire_kind && last->wire_n == f.wire_n && last->tail == f.tail) {
        last->gate_end = f.gate_end;
        last->var_end = f.var_end;
        last->items += f.items;
    } else {
        if (only_if_long && f.gate_end - f.gate_base < pg::kFootprintMinRows) return;
        if (only_if_long && last && last->gate_end > f.gate_base) return;  // (footprints stay in row order; cannot happen: flushes go in call order)
        c->segs.push_back(f);
    }
    c->sparse_hint += f.items * pg::kind_sparse_hint(f.wire_kind);  // references to Variables created before the call
}

// a queued gadget call (Queued::kind 1: range_check, 2: max_bound) as a kind of footprint, and what it weighs (footprint.hpp); a fused
// pair's first Variable is its witness
static_assert(pg::WIRES_RANGE_CHECK == 1 && pg::WIRES_MAX_BOUND == 2, "Queued::kind is the wire kind of the fused call");
uint32_t gadget_kind(const pg_composer::Queued &q, bool fused) { return pg::ladder_kind(q.kind, fused); }
uint32_t gadget_rows(const pg_composer::Queued &q) { return pg::kind_rows(q.kind, q.num_bits); }
uint32_t gadget_vars(const pg_composer::Queued &q, bool fused) { return pg::kind_vars(gadget_kind(q, fused), q.num_bits); }

// a run of `count` queued gadget calls of one kind and one set of public bounds starting at queue[i]; fused = each is
// preceded by the add_input that allocated its witness (the reference's loop: allocate, then range_check -- stride 2)
pg_status flush_gadgets(pg_composer *c, size_t i, size_t count, bool fused, size_t gates_between = 0) {
    // gates_between: that many rows-only gate calls follow every gadget call of the run (the loop of the reference's tests: allocate,
    // range_check, constrain_to_constant on the result) -- the items' rows are that many rows apart, their Variables are not
    const size_t stride = (fused ? 2 : 1) + gates_between, at = fused ? i + 1 : i;
    const pg_composer::Queued &q0 = c->queue[at];
    // staging: witness assignments (32 B each), then their Variables (8 B each)
    const size_t bytes = count * 40;
    char *h, *d;
    queue_slice(c, bytes, &h, &d);
    uint64_t *host = reinterpret_cast<uint64_t *>(h);
    for (size_t k = 0; k < count; k++) {
        const pg_composer::Queued &q = c->queue[at + k * stride];
        std::memcpy(&host[4 * k], q.wval.l, 32);
        host[4 * count + k] = q.wvar;
    }
    PG_HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    const pg_scalar *d_wit = reinterpret_cast<const pg_scalar *>(d);
    const pg_variable *d_var = reinterpret_cast<const pg_variable *>(reinterpret_cast<const uint64_t *>(d) + 4 * count);
    const uint64_t gate0 = q0.gate, var0 = fused ? c->queue[i].g.var : q0.var;
    const pg_columns out = cols_at(c, gate0, var0);
    pg_scalar mn, mx;
    from_fr(q0.b0, &mn);
    from_fr(q0.b1, &mx);
    pg_status st;
    const bool values_only = q0.in_place;  // (a run is of one kind in this too: same_gadget)
    const uint32_t stride_rows = gates_between ? gadget_rows(q0) + (uint32_t)gates_between : 0u;
    if (q0.kind == 1)
        st = range_check_common(c->e, &mn, &mx, fused ? nullptr : d_var, d_wit, count, gate0, var0, &out, nullptr, c->stream, values_only,
                                stride_rows);
    else
        st = max_bound_common(c->e, &mx, fused ? nullptr : d_var, d_wit, count, gate0, var0, &out, nullptr, c->stream, values_only, stride_rows);
    c->flush_launches++;
    if (st == PG_OK && !gates_between) add_footprint(c, pg::footprint(gate0, var0, count, gadget_kind(q0, fused), q0.num_bits), true);
    return st;
}

bool same_gadget(const pg_composer::Queued &a, const pg_composer::Queued &b) {
    return a.kind == b.kind && a.num_bits == b.num_bits && a.in_place == b.in_place && pg::fr_eq(a.b0, b.b0) && pg::fr_eq(a.b1, b.b1);
}
// queue[i] is an add_input and queue[i + 1] a gadget call on exactly the Variable / assignment it allocated
bool fused_pair(const pg_composer *c, size_t i) {
    if (i + 1 >= c->queue.size()) return false;
    const pg_composer::Queued &a = c->queue[i], &g = c->queue[i + 1];
    return a.kind == 0 && a.g.op == pg::OP_ADD_INPUT && g.kind != 0 && g.wvar == a.g.var && pg::fr_eq(g.wval, a.g.value) &&
           g.var == a.g.var + 1;
}

// A LOOP BODY at queue[i]: a gadget call -- with the allocate of its witness in front of it (fused) or on a witness allocated earlier --
// followed by g rows-only gate calls (one row each, no Variable created: constrain_to_constant, assert_equal, boolean_gate, poly_gate).
// how many such gates follow the body's gadget call (at most 8)
size_t loop_gates(const pg_composer *c, size_t i, bool fused) {
    const size_t first = i + (fused ? 2 : 1);
    size_t g = 0;
    while (g < 8 && first + g < c->queue.size() && c->queue[first + g].kind == 0 && c->queue[first + g].g.op == pg::OP_ROW) g++;
    return g;
}
bool body_at(const pg_composer *c, size_t i, bool fused) {
    return fused ? fused_pair(c, i) : (i < c->queue.size() && c->queue[i].kind != 0);
}
// body number `k` of a loop that starts at queue[i] lies where the stride says: rows L + g apart, Variables as many as a body creates
bool same_stride(const pg_composer *c, size_t i, size_t body, size_t k, bool fused) {
    const size_t go = fused ? 1 : 0;
    const pg_composer::Queued &a = c->queue[i + go], &b = c->queue[i + body * k + go], &p = c->queue[i + body * (k - 1) + go];
    const uint64_t rows = gadget_rows(a) + (body - 1 - go);
    return b.gate == a.gate + k * rows && b.gate - p.gate == rows && b.var - p.var == gadget_vars(a, fused);
}
// The loop at queue[i], if there is one (>= 2 bodies of the same gadget, bounds, gate count and stride): the gadget calls as ONE launch
// whose items lie g rows apart, then the gates as one run -- a row's place was assigned when its call was recorded, and a rows-only gate
// reads no assignment, so the order of the launches is free.  Without this every gadget call of such a loop is a launch of its own:
// 33-43 us per iteration against 3-5.  Returns the number of queue entries taken (0: no loop here).
size_t flush_loop(pg_composer *c, size_t i, bool fused, pg_status *st) {
    if (!body_at(c, i, fused)) return 0;
    const size_t g = loop_gates(c, i, fused), go = fused ? 1 : 0;
    if (!g) return 0;
    const size_t body = 1 + go + g;
    size_t count = 1;
    while (body_at(c, i + body * count, fused) && same_gadget(c->queue[i + go], c->queue[i + body * count + go]) &&
           loop_gates(c, i + body * count, fused) >= g && same_stride(c, i, body, count, fused))
        count++;
    if (count < 2) return 0;
    *st = flush_gadgets(c, i, count, fused, g);
    std::vector<size_t> gates;
    gates.reserve(count * g);
    for (size_t k = 0; k < count; k++)
        for (size_t m = 0; m < g; m++) gates.push_back(i + body * k + 1 + go + m);
    if (*st == PG_OK) *st = flush_gate_list(c, gates);
    if (*st == PG_OK) {
        // every one of those gates on the gadget's own RESULT, three times (constrain_to_constant / boolean_gate on what the call
        // returned): then the body is an item of rows + g rows whose wires are closed forms throughout, and the f-rows may know it
        // (PermSeg::tail)
        const pg_composer::Queued &q0 = c->queue[i + go];
        const uint32_t vars = gadget_vars(q0, fused);
        bool own_result = true;
        for (size_t k = 0; k < count && own_result; k++) {
            const uint64_t first_var = fused ? c->queue[i + body * k].g.var : c->queue[i + body * k].var;
            const uint64_t res = first_var + vars - 1;
            for (size_t m = 0; m < g; m++) {
                const pg::GateCmd &gc = c->queue[i + body * k + 1 + go + m].g;
                own_result = own_result && gc.a == res && gc.b == res && gc.c == res;
            }
        }
        if (own_result)
            add_footprint(c, pg::footprint(q0.gate, fused ? c->queue[i].g.var : q0.var, count, gadget_kind(q0, fused), q0.num_bits, (uint32_t)g), true);
    }
    return body * count;
}

// everything recorded so far goes to the composer's stream, in order, as few launches as the order allows
pg_status flush(pg_composer *c) {
    if (c->queue.empty()) return PG_OK;
    PG_HIP_TRY(hipSetDevice(c->e->device));
    const size_t N = c->queue.size();
    PG_TRY(queue_begin(c, N));
    pg_status st = PG_OK;
    size_t i = 0;
    while (i < N && st == PG_OK) {
        // a loop with gates behind every gadget call (the allocate in front of the call, or the witnesses allocated earlier)
        if (const size_t taken = flush_loop(c, i, fused_pair(c, i), &st)) {
            i += taken;
            continue;
        }
        if (fused_pair(c, i)) {  // allocate + gadget, repeated with the same public bounds: ONE batched launch
            size_t count = 1;
            while (fused_pair(c, i + 2 * count) && same_gadget(c->queue[i + 1], c->queue[i + 2 * count + 1])) count++;
            st = flush_gadgets(c, i, count, true);
            i += 2 * count;
        } else if (c->queue[i].kind == 0) {
            size_t j = i + 1;
            while (j < N && c->queue[j].kind == 0 && !fused_pair(c, j)) j++;
            st = flush_gates(c, i, j);
            i = j;
        } else {  // gadget calls on witnesses allocated earlier
            size_t count = 1;
            while (i + count < N && c->queue[i + count].kind != 0 && same_gadget(c->queue[i], c->queue[i + count])) count++;
            st = flush_gadgets(c, i, count, false);
            i += count;
        }
    }
    c->queue.clear();
    c->flushes++;
    if (c->staging[c->stage].sent(c->stream) != hipSuccess && st == PG_OK) st = fail(PG_ERR_HIP, "recording the flush's event failed");
    return st;
}

pg_status run_gate(pg_composer *c, const pg::GateCmd &cmd_in) {
    pg::GateCmd cmd = cmd_in;
    if (c->queueing && c->queue.size() >= PG_QUEUE_MAX) PG_TRY(flush(c));  // (before the decision: a flush can fail)
    // a row: selectors, wires, where it lands (and its public input: it enters the output's value); add_input leaves no signature
    SigHasher h;
    h.u64(cmd.op); h.u64(cmd.gate); h.u64(cmd.var); h.u64(cmd.a); h.u64(cmd.b); h.u64(cmd.c);
    h.fr(cmd.q_m); h.fr(cmd.q_l); h.fr(cmd.q_r); h.fr(cmd.q_o); h.fr(cmd.q_c); h.fr(cmd.pi);
    SignedAppend sa(c, h.done(), 1, cmd.op != pg::OP_ADD_INPUT);
    if (c->queueing) {
        c->queue.emplace_back();
        c->queue.back().kind = 0;
        c->queue.back().g = cmd;
        c->queue.back().in_place = sa.in_place;
        sa.commit();
        return PG_OK;
    }
    if (sa.in_place) cmd.op |= pg::OP_ROW_IN_PLACE;
    PG_HIP_TRY(hipSetDevice(c->e->device));
    hipLaunchKernelGGL(pg::gate_kernel, dim3(1), dim3(64), 0, c->stream, cmd, c->cols.view());
    PG_HIP_TRY(hipGetLastError());
    sa.commit();
    return PG_OK;
}

pg::Fr opt_fr(const pg_scalar *s) { return s ? to_fr(s) : pg::fr_zero(); }

// append one arithmetic row (poly_gate and friends).  w_4 = zero_var, q_4 = 0, q_arith = 1.
pg_status push_row(pg_composer *c, pg_variable a, pg_variable b, pg_variable o, const pg::Fr &q_m, const pg::Fr &q_l,
                   const pg::Fr &q_r, const pg::Fr &q_o, const pg::Fr &q_c, const pg_scalar *pi) {
    PG_TRY(need(c, 1, 0));
    PG_TRY(check_var(c, a));
    PG_TRY(check_var(c, b));
    PG_TRY(check_var(c, o));
    pg::GateCmd cmd{};
    cmd.op = pg::OP_ROW;
    cmd.gate = c->n;
    cmd.a = a; cmd.b = b; cmd.c = o;
    cmd.q_m = q_m; cmd.q_l = q_l; cmd.q_r = q_r; cmd.q_o = q_o; cmd.q_c = q_c;
    cmd.pi = pg::fr_zero();
    PG_TRY(run_gate(c, cmd));
    if (pi) { c->pi_gate.push_back(c->n); c->pi_val.push_back(*pi); }
    c->n += 1;
    return PG_OK;
}

pg_status stage(pg_composer *c, const pg::StageBlob &blob, uint32_t words) {
    hipLaunchKernelGGL(pg::stage_kernel, dim3(1), dim3(64), 0, c->stream, blob, c->stage_words(), words);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

void blob_scalar(pg::StageBlob &b, int word, const pg_scalar *s) { std::memcpy(&b.w[word], s->l, 32); }


}  // namespace

extern "C" {

pg_status pg_composer_create(pg_engine *e, uint64_t gate_capacity, uint64_t var_capacity, int with_dummy, void *stream,
                             pg_composer **out) {
    if (!e || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (gate_capacity < 3 || var_capacity < 5) return fail(PG_ERR_INVALID_ARGUMENT, "capacity below the initial state");
    PG_HIP_TRY(hipSetDevice(e->device));
    // (on every failing way out: pg_composer_destroy, which drains the stream before the members go)
    std::unique_ptr<pg_composer, void (*)(pg_composer *)> owner(new (std::nothrow) pg_composer(), pg_composer_destroy);
    pg_composer *c = owner.get();
    if (!c) return fail(PG_ERR_HIP, "out of host memory");
    c->e = e;
    c->stream = static_cast<hipStream_t>(stream);
    if (c->cols.create(gate_capacity, var_capacity) != PG_OK || c->d_stage.reserve(sizeof(pg::StageBlob)) != PG_OK ||
        c->d_preflight.reserve(sizeof(pg::Preflight)) != PG_OK)
        return fail(PG_ERR_HIP, "hipMalloc of the composer columns failed");
    PG_TRY(c->h_total.reserve(sizeof(pg::Preflight)));
    // StandardComposer::new(): zero_var = add_witness_to_circuit_description(0), then add_dummy_constraints()
    pg_scalar zero, s;
    from_fr(pg::fr_zero(), &zero);
    pg_status st = pg_composer_add_witness_to_circuit_description(c, &zero, &c->zero_var);
    if (st == PG_OK && with_dummy) {
        pg_variable six, one, seven, m20;
        pg_scalar_from_u64(6, &s); st = pg_composer_add_input(c, &s, &six);
        pg_scalar_from_u64(1, &s); if (st == PG_OK) st = pg_composer_add_input(c, &s, &one);
        pg_scalar_from_u64(7, &s); if (st == PG_OK) st = pg_composer_add_input(c, &s, &seven);
        from_fr(pg::fr_neg(pg::fr_from_u64(20)), &s); if (st == PG_OK) st = pg_composer_add_input(c, &s, &m20);
        if (st == PG_OK) {
            // (6, 7, -20, 1 ; 1, 2, 3, 4, 4 ; q_4 = 1 on w_4 = `one`)
            st = push_row(c, six, seven, m20, pg::fr_from_u64(1), pg::fr_from_u64(2), pg::fr_from_u64(3), pg::fr_from_u64(4),
                          pg::fr_from_u64(4), nullptr);
            if (st == PG_OK) c->fourth.push_back(pg::FourthWire{c->n - 1, one, pg::fr_one()});
        }
        if (st == PG_OK)  // (-20, 6, 7, zero ; 1, 1, 1, 1, 127)
            st = push_row(c, m20, six, seven, pg::fr_from_u64(1), pg::fr_from_u64(1), pg::fr_from_u64(1), pg::fr_from_u64(1),
                          pg::fr_from_u64(127), nullptr);
    }
    if (st != PG_OK) return st;
    c->n0 = c->n;
    c->nvars0 = c->nvars;
    c->log0 = c->log.size();
    c->fourth0 = c->fourth.size();
    c->rows_rewritten = 0;
    *out = owner.release();
    return PG_OK;
}

// Prover::clear_witness() of the reference's tests (tests/scalar_gadgets_tests.rs:110,170,228): the composer is a fresh one
// again -- StandardComposer::new()'s state -- and the circuit is rebuilt by the same calls with other witnesses.  The device
// columns stay where they are: an append that repeats what the previous build did at the same place (pg_composer::log)
// finds its rows in place and writes only its assignments.
pg_status pg_composer_clear_witness(pg_composer *c) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));  // what was recorded belongs to the build that ends here
    PG_HIP_TRY(hipSetDevice(c->e->device));
    if (!c->ragged.empty()) {  // the prefix sums of ragged calls, referenced by the footprints that go now
        PG_HIP_TRY(hipStreamSynchronize(c->stream));
        c->ragged.clear();
    }
    if (!c->refill || c->n > c->old_n) c->old_n = c->n;  // (a refresh that stopped early leaves the rest of the older build in place)
    c->n = c->n0;
    c->nvars = c->nvars0;
    c->pi_gate.clear();
    c->pi_val.clear();
    c->fourth.resize(c->fourth0);
    c->range_segs.clear();
    c->segs.clear();
    c->sparse_hint = 0;
    c->last_kind = 0;
    c->cursor = c->log0;
    c->refill = c->log.size() > c->log0;
    c->rows_in_place = c->rows_rewritten = 0;
    return PG_OK;
}

pg_status pg_composer_refresh_stats(const pg_composer *c, uint64_t *rows_in_place, uint64_t *rows_rewritten, int *refreshing) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    if (rows_in_place) *rows_in_place = c->rows_in_place;
    if (rows_rewritten) *rows_rewritten = c->rows_rewritten;
    if (refreshing) *refreshing = c->refill ? 1 : 0;
    return PG_OK;
}

// ordering only: the engine's device current, the composer's stream drained.  The members release themselves.
void pg_composer_destroy(pg_composer *c) {
    if (!c) return;
    (void)hipSetDevice(c->e->device);
    (void)hipStreamSynchronize(c->stream);
    delete c;
}

uint64_t pg_composer_circuit_size(const pg_composer *c) { return c ? c->n : 0; }
uint64_t pg_composer_num_variables(const pg_composer *c) { return c ? c->nvars : 0; }
pg_variable pg_composer_zero_var(const pg_composer *c) { return c ? c->zero_var : 0; }

pg_status pg_composer_columns(const pg_composer *c, pg_columns *out) {
    if (!c || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(flush(const_cast<pg_composer *>(c)));  // what was recorded is on the stream before anybody reads the columns
    *out = cols_at(c, 0, 0);
    return PG_OK;
}

pg_status pg_composer_reserve(pg_composer *c, uint64_t gate_capacity, uint64_t var_capacity) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    return grow(c, gate_capacity, var_capacity);
}
pg_status pg_composer_spread_columns(pg_composer *c, uint64_t stride_bytes) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    if (stride_bytes > (1ull << 44)) return fail(PG_ERR_INVALID_ARGUMENT, "stride too large");
    return grow(c, 0, 0, stride_bytes);  // (when it fails the composer keeps its buffers and its layout)
}
pg_status pg_composer_auto_grow(pg_composer *c, int on) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    c->auto_grow = on != 0;
    return PG_OK;
}
uint64_t pg_composer_gate_capacity(const pg_composer *c) { return c ? c->cols.gate_cap() : 0; }
uint64_t pg_composer_var_capacity(const pg_composer *c) { return c ? c->cols.var_cap() : 0; }

pg_status pg_composer_queue(pg_composer *c, int on) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    if (!on) PG_TRY(flush(c));
    c->queueing = on != 0;
    return PG_OK;
}

pg_status pg_composer_flush(pg_composer *c) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    return flush(c);
}

pg_status pg_composer_queue_stats(const pg_composer *c, uint64_t *pending, uint64_t *flushes, uint64_t *launches) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    if (pending) *pending = c->queue.size();
    if (flushes) *flushes = c->flushes;
    if (launches) *launches = c->flush_launches;
    return PG_OK;
}

pg_status pg_composer_sync(pg_composer *c) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));
    PG_HIP_TRY(hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_composer_add_input(pg_composer *c, const pg_scalar *s, pg_variable *out) {
    if (!s || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(need(c, 0, 1));
    if (!is_reduced(to_fr(s))) return fail(PG_ERR_INVALID_ARGUMENT, "scalar is not a reduced BlsScalar");
    pg::GateCmd cmd{};
    cmd.op = pg::OP_ADD_INPUT;
    cmd.var = c->nvars;
    cmd.value = to_fr(s);
    PG_TRY(run_gate(c, cmd));
    *out = c->nvars++;
    return PG_OK;
}

pg_status pg_composer_poly_gate(pg_composer *c, pg_variable a, pg_variable b, pg_variable o, const pg_scalar *q_m,
                                const pg_scalar *q_l, const pg_scalar *q_r, const pg_scalar *q_o, const pg_scalar *q_c,
                                const pg_scalar *pi) {
    if (!c || !q_m || !q_l || !q_r || !q_o || !q_c) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return push_row(c, a, b, o, to_fr(q_m), to_fr(q_l), to_fr(q_r), to_fr(q_o), to_fr(q_c), pi);
}

pg_status pg_composer_constrain_to_constant(pg_composer *c, pg_variable a, const pg_scalar *constant, const pg_scalar *pi) {
    if (!c || !constant) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    // poly_gate(a, a, a, 0, 1, 0, 0, -constant, pi)
    return push_row(c, a, a, a, pg::fr_zero(), pg::fr_one(), pg::fr_zero(), pg::fr_zero(), pg::fr_neg(to_fr(constant)), pi);
}

pg_status pg_composer_add_witness_to_circuit_description(pg_composer *c, const pg_scalar *value, pg_variable *out) {
    if (!value || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(need(c, 1, 1));
    PG_TRY(pg_composer_add_input(c, value, out));
    return pg_composer_constrain_to_constant(c, *out, value, nullptr);
}

pg_status pg_composer_assert_equal(pg_composer *c, pg_variable a, pg_variable b) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    // poly_gate(a, b, zero_var, 0, 1, -1, 0, 0, None)
    return push_row(c, a, b, c->zero_var, pg::fr_zero(), pg::fr_one(), pg::fr_neg_one(), pg::fr_zero(), pg::fr_zero(), nullptr);
}

static pg_status add_or_mul(pg_composer *c, uint32_t op, const pg::Fr &q_m, const pg::Fr &q_l, const pg::Fr &q_r, pg_variable a,
                            pg_variable b, const pg_scalar *q_c, const pg_scalar *pi, pg_variable *out) {
    if (!c || !q_c || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(need(c, 1, 1));
    PG_TRY(check_var(c, a));
    PG_TRY(check_var(c, b));
    pg::GateCmd cmd{};
    cmd.op = op;
    cmd.gate = c->n;
    cmd.var = c->nvars;
    cmd.a = a; cmd.b = b;
    cmd.q_m = q_m; cmd.q_l = q_l; cmd.q_r = q_r;
    cmd.q_o = pg::fr_neg_one();
    cmd.q_c = to_fr(q_c);
    cmd.pi = opt_fr(pi);
    PG_TRY(run_gate(c, cmd));
    if (pi) { c->pi_gate.push_back(c->n); c->pi_val.push_back(*pi); }
    c->n += 1;
    *out = c->nvars++;
    return PG_OK;
}

pg_status pg_composer_add(pg_composer *c, const pg_scalar *q_l, pg_variable a, const pg_scalar *q_r, pg_variable b,
                          const pg_scalar *q_c, const pg_scalar *pi, pg_variable *out) {
    if (!q_l || !q_r) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return add_or_mul(c, pg::OP_ADD, pg::fr_zero(), to_fr(q_l), to_fr(q_r), a, b, q_c, pi, out);
}

pg_status pg_composer_mul(pg_composer *c, const pg_scalar *q_m, pg_variable a, pg_variable b, const pg_scalar *q_c,
                          const pg_scalar *pi, pg_variable *out) {
    if (!q_m) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return add_or_mul(c, pg::OP_MUL, to_fr(q_m), pg::fr_zero(), pg::fr_zero(), a, b, q_c, pi, out);
}

pg_status pg_composer_mul_gate(pg_composer *c, pg_variable a, pg_variable b, pg_variable o, const pg_scalar *q_m,
                               const pg_scalar *q_o, const pg_scalar *q_c, const pg_scalar *pi) {
    if (!c || !q_m || !q_o || !q_c) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return push_row(c, a, b, o, to_fr(q_m), pg::fr_zero(), pg::fr_zero(), to_fr(q_o), to_fr(q_c), pi);
}

pg_status pg_composer_boolean_gate(pg_composer *c, pg_variable a) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    return push_row(c, a, a, a, pg::fr_one(), pg::fr_zero(), pg::fr_zero(), pg::fr_neg_one(), pg::fr_zero(), nullptr);
}

/* ---- the reference's public API on a composer ------------------------------------------------ */

pg_status pg_allocated_scalar_allocate(pg_composer *c, const pg_scalar *scalar, pg_allocated_scalar *out) {
    if (!scalar || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(pg_composer_add_input(c, scalar, &out->var));
    out->scalar = *scalar;
    return PG_OK;
}

// The two ladder gadgets called one at a time on an allocated witness: recorded on the queue (flushed together with their neighbours:
// consecutive calls with the same bounds are one launch) or launched as a batch of one.  kind: the call's SigKind, Queued::kind and
// pg_composer::last_kind in one; min_range: NULL for max_bound (zero wherever the call's pair of bounds is kept).
static pg_status single_ladder(pg_composer *c, SigKind kind, const pg_scalar *min_range, const pg_scalar *max_range,
                               const pg_allocated_scalar *witness, pg_variable *out, uint64_t *num_bits) {
    const bool range_check = kind == SigKind::RANGE_CHECK;
    if (!c || !witness || !out || !max_range || (range_check && !min_range)) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    const pg_scalar mn = range_check ? *min_range : pg_scalar{};
    if (!(c->last_kind == (int)kind && std::memcmp(&c->last_min, &mn, 32) == 0 && std::memcmp(&c->last_max, max_range, 32) == 0)) {
        c->last_kind = 0;
        PG_TRY(range_check ? pg_range_check_layout(&mn, max_range, 1, &c->last_lay) : pg_max_bound_layout(max_range, 1, &c->last_lay));
        c->last_min = mn;
        c->last_max = *max_range;
        c->last_kind = (int)kind;
    }
    const pg_layout lay = c->last_lay;
    // (the witness is already allocated: the `_allocated` twin's Variables)
    const uint64_t rows = lay.gates_per_item, vars = pg::kind_vars(pg::ladder_kind((uint32_t)kind, false), lay.num_bits);
    PG_TRY(need(c, rows, vars));
    PG_TRY(check_var(c, witness->var));
    if (!is_reduced(to_fr(&witness->scalar))) return fail(PG_ERR_INVALID_ARGUMENT, "witness is not a reduced BlsScalar");
    if (range_check && (lay.num_bits < 2 || lay.num_bits > 255)) return fail(PG_ERR_INVALID_ARGUMENT, "ladder length out of range");
    // the rows: a function of the bounds, the witness VARIABLE and where the call lands
    if (c->queueing && c->queue.size() >= PG_QUEUE_MAX) PG_TRY(flush(c));  // (before the decision: a flush can fail)
    SignedAppend sa(c, gadget_sig(c, kind, to_fr(&mn), to_fr(max_range), 1, witness->var), rows);
    if (c->queueing) {
        c->queue.emplace_back();
        pg_composer::Queued &q = c->queue.back();
        q.in_place = sa.in_place;
        q.kind = (uint8_t)kind;
        q.b0 = to_fr(&mn);
        q.b1 = to_fr(max_range);
        q.num_bits = (uint32_t)lay.num_bits;
        q.wvar = witness->var;
        q.wval = to_fr(&witness->scalar);
        q.gate = c->n;
        q.var = c->nvars;
    } else {
        pg::StageBlob b{};
        blob_scalar(b, 0, &witness->scalar);
        b.w[4] = witness->var;
        PG_TRY(stage(c, b, 5));
        const pg_columns at = cols_at(c, c->n, c->nvars);
        const auto one_item = [&](auto gd, auto A) {  // what the two gadgets' Args share; the batch of one
            A.max_range = to_fr(max_range);
            A.n = (uint32_t)lay.num_bits;
            A.witness = reinterpret_cast<const uint4 *>(c->stage_words());
            A.witness_vars = c->stage_words() + 4;
            A.pow2 = c->e->d_pow2.as<uint4>();
            return launch<decltype(gd)>(c->e, A, &at, 1, c->n, c->nvars, c->zero_var, nullptr, nullptr, c->stream, nullptr, sa.in_place);
        };
        if (range_check) {
            pg::RangeCheckGD::Args A{};
            A.min_range = to_fr(&mn);
            PG_TRY(one_item(pg::RangeCheckGD{}, A));
        } else {
            PG_TRY(one_item(pg::MaxBoundGD<false>{}, pg::MaxBoundGD<false>::Args{}));
        }
    }
    sa.commit();
    c->n += rows;
    c->nvars += vars;
    *out = c->nvars - 1;  // composer.mul(1, y1, y2, 0) is the last variable, range.rs:42
    if (num_bits) *num_bits = lay.num_bits;
    return PG_OK;
}
static_assert((uint32_t)SigKind::RANGE_CHECK == pg::WIRES_RANGE_CHECK && (uint32_t)SigKind::MAX_BOUND == pg::WIRES_MAX_BOUND,
              "a single ladder call's SigKind is its Queued::kind, the wire kind of the fused call");

pg_status pg_range_check(pg_composer *c, const pg_scalar *min_range, const pg_scalar *max_range,
                         const pg_allocated_scalar *witness, pg_variable *out) {
    return single_ladder(c, SigKind::RANGE_CHECK, min_range, max_range, witness, out, nullptr);
}

pg_status pg_max_bound(pg_composer *c, const pg_scalar *max_range, const pg_allocated_scalar *witness, pg_variable *out,
                       uint64_t *num_bits) {
    return single_ladder(c, SigKind::MAX_BOUND, nullptr, max_range, witness, out, num_bits);
}

pg_status pg_scalar_decomposition_gadget(pg_composer *c, uint64_t num_bits, const pg_allocated_scalar *witness,
                                         pg_variable *is_equal, pg_variable *bits_out) {
    if (!c || !witness || !is_equal) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(flush(c));
    pg_layout lay;
    PG_TRY(pg_scalar_decomposition_layout(num_bits, 1, &lay));
    PG_TRY(need(c, lay.n_gates, lay.n_vars));
    PG_TRY(check_var(c, witness->var));
    if (!is_reduced(to_fr(&witness->scalar))) return fail(PG_ERR_INVALID_ARGUMENT, "witness is not a reduced BlsScalar");
    pg::StageBlob b{};
    blob_scalar(b, 0, &witness->scalar);
    b.w[4] = witness->var;
    PG_TRY(stage(c, b, 5));
    const pg_columns at = cols_at(c, c->n, c->nvars);
    SignedAppend sa(c, gadget_sig(c, SigKind::DECOMPOSITION, pg::fr_zero(), pg::fr_zero(), num_bits, witness->var), lay.n_gates);
    PG_TRY(decomposition_common(c->e, num_bits, c->stage_words() + 4, reinterpret_cast<const pg_scalar *>(c->stage_words()), 1, c->n, c->nvars, &at,
                                nullptr, c->stream, sa.in_place));
    sa.commit();
    if (bits_out)
        for (uint64_t i = 0; i < num_bits; i++) bits_out[i] = c->nvars + i;
    c->n += lay.n_gates;
    c->nvars += lay.n_vars;
    *is_equal = c->nvars - 1;
    return PG_OK;
}

// The four scalar gadgets, called one at a time, ARE sequences of composer calls (src/scalar.rs) -- and the composer's gate calls are
// recorded, not launched (the command queue above): so these are composed here from those very calls, in the reference's order, and a
// loop of them costs what a loop of gate calls costs.  (Until the end of round 5 each was a one-item launch of its batched emitter behind
// a flush: 13 us per select, 45 us per maybe_equal / is_non_zero.)  Assignments: an output of add / mul is computed on the device from
// its operands' assignments; what needs the host's arithmetic -- the inverse -- is allocated with its value, as the reference does.
namespace {
pg_scalar scalar_of(const pg::Fr &f) {
    pg_scalar s;
    from_fr(f, &s);
    return s;
}
}  // namespace

pg_status pg_conditionally_select_zero(pg_composer *c, pg_variable x, pg_variable select, pg_variable *out) {
    if (!c || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(need(c, 1, 1));
    PG_TRY(check_var(c, x));
    PG_TRY(check_var(c, select));
    const pg_scalar one = scalar_of(pg::fr_one()), zero = scalar_of(pg::fr_zero());
    return pg_composer_mul(c, &one, x, select, &zero, nullptr, out);  // scalar.rs:21-27: x * select
}

pg_status pg_conditionally_select_one(pg_composer *c, pg_variable y, pg_variable selector, pg_variable *out) {
    if (!c || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(need(c, 4, 4));
    PG_TRY(check_var(c, y));
    PG_TRY(check_var(c, selector));
    const pg_scalar one = scalar_of(pg::fr_one()), zero = scalar_of(pg::fr_zero()), neg_one = scalar_of(pg::fr_neg_one());
    pg_variable one_v, selector_y, one_min_selector;
    PG_TRY(pg_composer_add_witness_to_circuit_description(c, &one, &one_v));                       // scalar.rs:41
    PG_TRY(pg_composer_mul(c, &one, y, selector, &zero, nullptr, &selector_y));                    // :43   s * y
    PG_TRY(pg_composer_add(c, &one, one_v, &neg_one, selector, &zero, nullptr, &one_min_selector));  // :45-50  1 - s
    return pg_composer_add(c, &one, selector_y, &one, one_min_selector, &zero, nullptr, out);      // :53-58  s y + (1 - s)
}

pg_status pg_maybe_equal(pg_composer *c, const pg_allocated_scalar *a, const pg_allocated_scalar *b, pg_variable *out) {
    if (!c || !a || !b || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_reduced(to_fr(&a->scalar)) || !is_reduced(to_fr(&b->scalar))) return fail(PG_ERR_INVALID_ARGUMENT, "scalar is not a reduced BlsScalar");
    PG_TRY(need(c, 3, 3));
    PG_TRY(check_var(c, a->var));
    PG_TRY(check_var(c, b->var));
    const pg_scalar one = scalar_of(pg::fr_one()), zero = scalar_of(pg::fr_zero()), neg_one = scalar_of(pg::fr_neg_one());
    pg_variable u, z, y;
    PG_TRY(pg_composer_add(c, &one, a->var, &neg_one, b->var, &zero, nullptr, &u));                 // scalar.rs:111-117  u = a - b
    const pg_scalar u_inv = scalar_of(pg::fr_invert_or_zero(pg::fr_sub(to_fr(&a->scalar), to_fr(&b->scalar))));  // :121-123  u^-1 or 0
    PG_TRY(pg_composer_add_input(c, &u_inv, &z));
    PG_TRY(pg_composer_mul(c, &neg_one, z, u, &one, nullptr, &y));                                  // :126  y = 1 - u z
    PG_TRY(pg_composer_mul_gate(c, y, u, u, &one, &zero, &zero, nullptr));                          // :129-138  y u = 0
    *out = y;
    return PG_OK;
}

pg_status pg_is_non_zero(pg_composer *c, pg_variable var, const pg_scalar *value_assigned) {
    if (!c || !value_assigned) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_reduced(to_fr(value_assigned))) return fail(PG_ERR_INVALID_ARGUMENT, "value is not a reduced BlsScalar");
    const bool err = pg::fr_is_zero(to_fr(value_assigned));  // scalar.rs:73-80
    PG_TRY(need(c, err ? 1 : 3, err ? 1 : 3));
    PG_TRY(check_var(c, var));
    pg_variable var_assigned, inv, one_v;
    PG_TRY(pg_composer_add_input(c, value_assigned, &var_assigned));  // :69
    PG_TRY(pg_composer_assert_equal(c, var, var_assigned));           // :71
    // (the reference returns its Err here, with the two calls above already in the circuit)
    if (err) return fail(PG_ERR_NON_EXISTING_INVERSE, "value_assigned has no inverse");
    const pg_scalar one = scalar_of(pg::fr_one()), zero = scalar_of(pg::fr_zero()), neg_one = scalar_of(pg::fr_neg_one());
    const pg_scalar inverse = scalar_of(pg::fr_invert_or_zero(to_fr(value_assigned)));
    PG_TRY(pg_composer_add_input(c, &inverse, &inv));                               // :77
    PG_TRY(pg_composer_add_witness_to_circuit_description(c, &one, &one_v));         // :83
    return pg_composer_poly_gate(c, var, inv, one_v, &one, &zero, &zero, &neg_one, &zero, nullptr);  // :84-94  var * inv - 1 = 0
}

static pg_status perm_reserve(pg_composer *c, Scratch &buf, size_t bytes);

}  // extern "C"

namespace {
// The uniform ladder batches: `batch` items of `wire_kind` at the composer's end.  layout: the call's pg_*_layout (ladder length, rows);
// emit: its *_common call; sig_kind, b0, b1: what its signature hashes beside the batch and the place.  A kind whose witnesses are
// Variables from elsewhere (the `_allocated` calls, decomposition) has their array checked and digested first.
template <class Layout, class Emit>
pg_status ladder_batch(pg_composer *c, uint32_t wire_kind, SigKind sig_kind, const pg::Fr &b0, const pg::Fr &b1, const pg_variable *d_witness_var,
                       uint64_t batch, uint64_t *num_bits, Layout layout, Emit emit) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));
    pg_layout lay;
    PG_TRY(layout(&lay));
    const uint64_t n_vars = pg::kind_vars(wire_kind, lay.num_bits) * batch;  // (an `_allocated` call: without the allocate's)
    pg_composer::Sig dg{0, 0};
    if (pg::ladder_foreign_per_item(wire_kind)) {
        if (batch) PG_TRY(check_u64s(d_witness_var, "d_witness_var"));
        PG_TRY(check_var_arrays(c, {d_witness_var}, batch, &dg));
    }
    PG_TRY(need(c, lay.n_gates, n_vars));
    const pg_columns at = cols_at(c, c->n, c->nvars);
    // (a witness refresh: the same call at the same place has left these rows here, pg_composer_clear_witness)
    SignedAppend sa(c, gadget_sig(c, sig_kind, b0, b1, batch, 0, dg), lay.n_gates, batch != 0);
    PG_TRY(emit(&at, sa.in_place));
    sa.commit();
    add_footprint(c, pg::footprint(c->n, c->nvars, batch, wire_kind, (uint32_t)lay.num_bits));
    c->n += lay.n_gates;
    c->nvars += n_vars;
    if (num_bits) *num_bits = lay.num_bits;
    return PG_OK;
}
pg_status range_check_batch(pg_composer *c, uint32_t wire_kind, SigKind sig_kind, const pg_scalar *min_range, const pg_scalar *max_range,
                            const pg_variable *d_witness_var, const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars) {
    return ladder_batch(
        c, wire_kind, sig_kind, opt_fr(min_range), opt_fr(max_range), d_witness_var, batch, nullptr,
        [&](pg_layout *lay) { return pg_range_check_layout(min_range, max_range, batch, lay); },
        [&](const pg_columns *at, bool in_place) {
            return range_check_common(c->e, min_range, max_range, d_witness_var, d_witness, batch, c->n, c->nvars, at, d_result_vars, c->stream, in_place);
        });
}
pg_status max_bound_batch(pg_composer *c, uint32_t wire_kind, SigKind sig_kind, const pg_scalar *max_range, const pg_variable *d_witness_var,
                          const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars, uint64_t *num_bits) {
    return ladder_batch(
        c, wire_kind, sig_kind, pg::fr_zero(), opt_fr(max_range), d_witness_var, batch, num_bits,
        [&](pg_layout *lay) { return pg_max_bound_layout(max_range, batch, lay); },
        [&](const pg_columns *at, bool in_place) {
            return max_bound_common(c->e, max_range, d_witness_var, d_witness, batch, c->n, c->nvars, at, d_result_vars, c->stream, in_place);
        });
}
}  // namespace

extern "C" {

pg_status pg_composer_range_check_batch(pg_composer *c, const pg_scalar *min_range, const pg_scalar *max_range,
                                        const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars) {
    return range_check_batch(c, pg::WIRES_RANGE_CHECK, SigKind::RANGE_CHECK_BATCH, min_range, max_range, nullptr, d_witness, batch, d_result_vars);
}
pg_status pg_composer_range_check_allocated_batch(pg_composer *c, const pg_scalar *min_range, const pg_scalar *max_range,
                                                  const pg_variable *d_witness_var, const pg_scalar *d_witness,
                                                  uint64_t batch, pg_variable *d_result_vars) {
    return range_check_batch(c, pg::WIRES_RANGE_CHECK_ALLOCATED, SigKind::RANGE_CHECK_ALLOCATED_BATCH, min_range, max_range, d_witness_var, d_witness, batch, d_result_vars);
}
pg_status pg_composer_max_bound_batch(pg_composer *c, const pg_scalar *max_range, const pg_scalar *d_witness, uint64_t batch,
                                      pg_variable *d_result_vars, uint64_t *num_bits) {
    return max_bound_batch(c, pg::WIRES_MAX_BOUND, SigKind::MAX_BOUND_BATCH, max_range, nullptr, d_witness, batch, d_result_vars, num_bits);
}
pg_status pg_composer_max_bound_allocated_batch(pg_composer *c, const pg_scalar *max_range, const pg_variable *d_witness_var,
                                                const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars,
                                                uint64_t *num_bits) {
    return max_bound_batch(c, pg::WIRES_MAX_BOUND_ALLOCATED, SigKind::MAX_BOUND_ALLOCATED_BATCH, max_range, d_witness_var, d_witness, batch, d_result_vars, num_bits);
}
pg_status pg_composer_scalar_decomposition_batch(pg_composer *c, uint64_t num_bits, const pg_variable *d_witness_var,
                                                 const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars) {
    return ladder_batch(
        c, pg::WIRES_DECOMPOSITION, SigKind::DECOMPOSITION_BATCH, pg::fr_from_u64(num_bits), pg::fr_zero(), d_witness_var, batch, nullptr,
        [&](pg_layout *lay) { return pg_scalar_decomposition_layout(num_bits, batch, lay); },
        [&](const pg_columns *at, bool in_place) {
            return decomposition_common(c->e, num_bits, d_witness_var, d_witness, batch, c->n, c->nvars, at, d_result_vars, c->stream, in_place);
        });
}

}  // extern "C"

namespace {
// dst[i] = the assignment of Variable d_var[i], from the composer's own table, on its stream (dst: in val_ws, sized by the caller)
pg_status gather_values(pg_composer *c, const pg_variable *d_var, uint64_t batch, pg_scalar *dst) {
    // (a lane moves 16 bytes, half an assignment: 2 * batch lanes' work)
    const uint64_t want = (2 * batch + pg::kThreads - 1) / pg::kThreads, most = (uint64_t)c->e->num_cus * 32;
    hipLaunchKernelGGL(pg::gather_wire_values_kernel, dim3((uint32_t)(want < most ? want : most)), dim3(pg::kThreads), 0, c->stream, d_var,
                       c->cols.view().vars, batch, reinterpret_cast<uint4 *>(dst));
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

// The appends on EXISTING Variables: `batch` items on the device arrays `arrays` (each with the name its errors give it), `rows` rows
// and `vars` Variables at the composer's end.  Assignments are gathered from the composer's own table into its scratch, then the
// engine call.
//   check(&dg)                    every entry a Variable of this composer, and the digest of the arrays (check_var_arrays, or the call's
//                                 own pass where other device arrays must be looked at in the same host synchronisation)
//   sign(dg)                      the call's signature
//   emit(&at, values, in_place)   its *_common call; values: the arrays' assignments, `batch` scalars per array in the list's order
//   record()                      what the composer remembers of the rows (a footprint, range items); n and nvars are still the call's first
template <class Check, class Sign, class Emit, class Record>
pg_status var_batch(pg_composer *c, std::initializer_list<std::pair<const pg_variable *, const char *>> arrays, uint64_t batch, uint64_t rows,
                    uint64_t vars, Check check, Sign sign, Emit emit, Record record) {
    PG_TRY(flush(c));
    if (batch == 0) return PG_OK;
    for (const auto &a : arrays) PG_TRY(check_u64s(a.first, a.second));
    pg_composer::Sig dg;
    PG_TRY(check(&dg));
    PG_TRY(need(c, rows, vars));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    PG_TRY(perm_reserve(c, c->val_ws, arrays.size() * batch * sizeof(pg_scalar)));
    pg_scalar *const values = c->val_ws.as<pg_scalar>();
    size_t i = 0;
    for (const auto &a : arrays) PG_TRY(gather_values(c, a.first, batch, values + batch * i++));
    const pg_columns at = cols_at(c, c->n, c->nvars);
    SignedAppend sa(c, sign(dg), rows);
    PG_TRY(emit(&at, values, sa.in_place));
    sa.commit();
    record();
    c->n += rows;
    c->nvars += vars;
    return PG_OK;
}

// the two-input scalar gadgets (the rows: the two Variable arrays and where the call lands)
template <class GD>
pg_status two_input_batch(pg_composer *c, SigKind kind, uint32_t wire_kind, const pg_variable *d_a_var, const pg_variable *d_b_var, uint64_t batch,
                          pg_variable *d_result_vars) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    return var_batch(
        c, {{d_a_var, "first Variable array"}, {d_b_var, "second Variable array"}}, batch, pg::kind_rows(wire_kind) * batch,
        pg::kind_vars(wire_kind) * batch, [&](pg_composer::Sig *dg) { return check_var_arrays(c, {d_a_var, d_b_var}, batch, dg); },
        [&](const pg_composer::Sig &dg) { return gadget_sig(c, kind, pg::fr_zero(), pg::fr_zero(), batch, 0, dg); },
        [&](const pg_columns *at, const pg_scalar *values, bool in_place) {
            return two_input_common<GD>(c->e, d_a_var, values, d_b_var, values + batch, batch, c->n, c->nvars, at, d_result_vars, c->stream, in_place);
        },
        [&] { add_footprint(c, pg::footprint(c->n, c->nvars, batch, wire_kind)); });
}

// the widget rows [first_row, first_row + items * (g + 1)): continue the last range segment or begin one
void note_range_items(pg_composer *c, uint64_t first_row, uint64_t items, uint32_t g) {
    pg::RangeSeg *last = c->range_segs.empty() ? nullptr : &c->range_segs.back();
    if (last && last->g == g && last->first + last->items * (g + 1) == first_row) last->items += items;
    else c->range_segs.push_back(pg::RangeSeg{first_row, items, g});
}

pg_status widget_num_bits(const char *gate, uint64_t most, uint64_t num_bits) {
    if (pg::widget_num_bits_ok(num_bits, most)) return PG_OK;
    return fail(PG_ERR_INVALID_ARGUMENT, std::string(gate) + ": num_bits must be even and in [2, " + std::to_string(most) + "], got " +
                                             std::to_string(num_bits));
}
pg_status range_num_bits(uint64_t num_bits) { return widget_num_bits("range_gate", pg::kRangeGateMaxBits, num_bits); }
pg_status interval_num_bits(uint64_t num_bits) { return widget_num_bits("interval_gate", pg::kIntervalGateMaxBits, num_bits); }

// the range widget on existing Variables (range_gate.hpp).  The rows leave no footprint (sigma and the wire values take the generic
// routes); the composer remembers where q_range = 1.  The rows: the Variable array, num_bits and where the call lands.
pg_status range_gate_batch(pg_composer *c, const pg_variable *d_witness_var, uint64_t num_bits, uint64_t batch) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(range_num_bits(num_bits));
    const pg::WidgetShape shape = pg::widget_shape(num_bits);
    return var_batch(
        c, {{d_witness_var, "d_witness_var"}}, batch, (uint64_t)shape.rows() * batch, (uint64_t)(shape.k - 1) * batch,
        [&](pg_composer::Sig *dg) { return check_var_arrays(c, {d_witness_var}, batch, dg); },
        [&](const pg_composer::Sig &dg) { return gadget_sig(c, SigKind::RANGE_GATE_BATCH, pg::fr_zero(), pg::fr_zero(), batch, num_bits, dg); },
        [&](const pg_columns *at, const pg_scalar *values, bool in_place) {
            return range_gate_common(c->e, d_witness_var, values, (uint32_t)num_bits, batch, c->n, c->nvars, c->zero_var, at, c->stream, in_place);
        },
        [&] { note_range_items(c, c->n, batch, shape.g); });
}

// the interval gadget on existing Variables (interval_gate.hpp): min <= witness <= max by two range widgets on the differences, whose
// terminal rows carry the subtractions.  d_min / d_max: device arrays with a pair of bounds per item, or NULL: *min, *max for the call.
// As range_gate_batch: assignments gathered from the composer's own table, no footprint, the widget rows remembered as 2 x batch
// range items of g + 1 rows.
// one public pair against the preconditions, as canonical integers
pg_status interval_bounds(const pg_scalar *min, const pg_scalar *max, uint64_t num_bits) {
    PG_TRY(check_field(min, "min"));
    PG_TRY(check_field(max, "max"));
    const pg::Fr lo = pg::fr_from_mont(to_fr(min)), hi = pg::fr_from_mont(to_fr(max));
    for (int k = 3; k >= 0; k--)
        if (lo.l[k] != hi.l[k]) {
            if (lo.l[k] > hi.l[k]) return fail(PG_ERR_INVALID_ARGUMENT, "interval_gate: min > max");
            break;
        }
    const pg::Fr top = pg::raw_shr(pg::fr_from_mont(pg::fr_sub(to_fr(max), to_fr(min))), (uint32_t)num_bits);
    if (top.l[0] | top.l[1] | top.l[2] | top.l[3])
        return fail(PG_ERR_INVALID_ARGUMENT, "interval_gate: max - min does not fit num_bits = " + std::to_string(num_bits) + " bits");
    return PG_OK;
}
// The preflight of the per-item form: the Variables' pass and ONE pass over the two bound arrays (interval_bounds_kernel), which
// leaves their digest and the items whose bounds violate the preconditions.
pg_status check_interval_arrays(pg_composer *c, const pg_variable *d_witness_var, const pg_scalar *d_min, const pg_scalar *d_max,
                                uint64_t num_bits, uint64_t batch, pg_composer::Sig *vars_dg, pg_composer::Sig *bounds_dg) {
    pg::Preflight r;
    PG_TRY(preflight(c, 1, r, [&](pg::Preflight *d) {
        digest_vars(c, d_witness_var, batch, d, 0);
        // (its waves end in contended atomics: interval_gate.hpp)
        hipLaunchKernelGGL(pg::interval_bounds_kernel, dim3(grid_cap((batch + pg::kThreads - 1) / pg::kThreads, (uint64_t)c->e->num_cus * 2)),
                           dim3(pg::kThreads), 0, c->stream, reinterpret_cast<const uint4 *>(d_min), reinterpret_cast<const uint4 *>(d_max),
                           batch, (uint32_t)num_bits, d);
    }));
    if (r.call[pg::kIntervalBadItems])
        return fail(PG_ERR_INVALID_ARGUMENT, "interval_gate: the bounds of " + std::to_string(r.call[pg::kIntervalBadItems]) +
                                                 " items are not reduced, have min > max or max - min beyond num_bits = " +
                                                 std::to_string(num_bits) + " bits; the first is item " + std::to_string(r.call[pg::kIntervalFirstBad]));
    *vars_dg = sig_of(r.vars);
    *bounds_dg = sig_of(r.others);
    return PG_OK;
}

pg_status interval_gate_batch(pg_composer *c, const pg_variable *d_witness_var, const pg_scalar *min, const pg_scalar *max,
                              const pg_scalar *d_min, const pg_scalar *d_max, uint64_t num_bits, uint64_t batch) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(interval_num_bits(num_bits));
    const bool per_item = !min;
    if (!per_item) PG_TRY(interval_bounds(min, max, num_bits));
    if ((batch + 255) / 256 > 0xffffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "batch too large for one call");
    const pg::WidgetShape shape = pg::widget_shape(num_bits);
    // what the signature has for the bounds: the uniform call's two scalars, or (b0's first words) the digest of the two arrays
    pg::Fr b0 = per_item ? pg::fr_zero() : to_fr(min), b1 = per_item ? pg::fr_zero() : to_fr(max);
    return var_batch(
        c, {{d_witness_var, "d_witness_var"}}, batch, 2 * (uint64_t)shape.rows() * batch, 2 * (uint64_t)shape.k * batch,
        [&](pg_composer::Sig *dg) -> pg_status {
            if (!per_item) return check_var_arrays(c, {d_witness_var}, batch, dg);
            PG_TRY(check_scalars(d_min, "d_min"));
            PG_TRY(check_scalars(d_max, "d_max"));
            pg_composer::Sig bounds;
            PG_TRY(check_interval_arrays(c, d_witness_var, d_min, d_max, num_bits, batch, dg, &bounds));
            b0.l[0] = bounds.a;
            b0.l[1] = bounds.b;
            return PG_OK;
        },
        [&](const pg_composer::Sig &dg) {
            return gadget_sig(c, per_item ? SigKind::INTERVAL_GATE_RAGGED_BATCH : SigKind::INTERVAL_GATE_BATCH, b0, b1, batch, num_bits, dg);
        },
        [&](const pg_columns *at, const pg_scalar *values, bool in_place) {
            return interval_gate_common(c->e, d_witness_var, values, b0, b1, per_item ? d_min : nullptr, per_item ? d_max : nullptr,
                                        (uint32_t)num_bits, batch, c->n, c->nvars, c->zero_var, at, c->stream, in_place);
        },
        [&] { note_range_items(c, c->n, 2 * batch, shape.g); });
}
// the comparison gadget on two arrays of existing Variables (compare_gate.hpp): result_vars[i] = the Variable that holds
// [x_i <= y_i] ([x_i < y_i] when strict) PROVIDED the circuit bounds both below 2^num_bits, as the first accumulator of one range
// widget over num_bits + 2 bits on 2^num_bits + y - x - strict.  As range_gate_batch: one preflight, assignments gathered from the
// composer's own table, no footprint, the widget rows remembered as range items.  The rows: both Variable arrays (which is x and
// which is y), num_bits, strict and where the call lands.
pg_status compare_num_bits(uint64_t num_bits) { return widget_num_bits("is_less_equal", pg::kCompareGateMaxBits, num_bits); }
pg_status is_less_equal_batch(pg_composer *c, const pg_variable *d_x_var, const pg_variable *d_y_var, uint64_t num_bits, bool strict,
                              uint64_t batch, pg_variable *d_result_vars) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(compare_num_bits(num_bits));
    const pg::WidgetShape shape = pg::compare_shape(num_bits);
    pg::Fr b0 = pg::fr_zero();  // (a word of the signature, not a scalar)
    b0.l[0] = strict ? 1 : 0;
    return var_batch(
        c, {{d_x_var, "d_x_var"}, {d_y_var, "d_y_var"}}, batch, (uint64_t)shape.rows() * batch, (uint64_t)shape.k * batch,
        [&](pg_composer::Sig *dg) -> pg_status {
            PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
            return check_var_arrays(c, {d_x_var, d_y_var}, batch, dg);
        },
        [&](const pg_composer::Sig &dg) { return gadget_sig(c, SigKind::IS_LESS_EQUAL_BATCH, b0, pg::fr_zero(), batch, num_bits, dg); },
        [&](const pg_columns *at, const pg_scalar *values, bool in_place) {
            return compare_gate_common(c->e, d_x_var, values, d_y_var, values + batch, (uint32_t)num_bits, strict, batch, c->n, c->nvars,
                                       c->zero_var, at, d_result_vars, c->stream, in_place);
        },
        [&] { note_range_items(c, c->n, batch, shape.g); });
}
// the single calls of the widgets are batches of one: the Variable goes through the composer's staging words
pg_status stage_variable(pg_composer *c, pg_variable witness) {
    PG_TRY(flush(c));
    PG_TRY(check_var(c, witness));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    pg::StageBlob b{};
    b.w[0] = witness;
    return stage(c, b, 1);
}
}  // namespace

extern "C" {

pg_status pg_composer_interval_gate_batch(pg_composer *c, const pg_variable *d_witness_var, const pg_scalar *min, const pg_scalar *max,
                                          uint64_t num_bits, uint64_t batch) {
    if (!min || !max) return fail(PG_ERR_INVALID_ARGUMENT, "interval_gate: min or max is NULL");
    return interval_gate_batch(c, d_witness_var, min, max, nullptr, nullptr, num_bits, batch);
}
pg_status pg_composer_interval_gate_ragged_batch(pg_composer *c, const pg_variable *d_witness_var, const pg_scalar *d_min,
                                                 const pg_scalar *d_max, uint64_t num_bits, uint64_t batch) {
    return interval_gate_batch(c, d_witness_var, nullptr, nullptr, d_min, d_max, num_bits, batch);
}
pg_status pg_composer_interval_gate(pg_composer *c, pg_variable witness, const pg_scalar *min, const pg_scalar *max, uint64_t num_bits) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    if (!min || !max) return fail(PG_ERR_INVALID_ARGUMENT, "interval_gate: min or max is NULL");
    PG_TRY(interval_num_bits(num_bits));
    PG_TRY(interval_bounds(min, max, num_bits));
    PG_TRY(stage_variable(c, witness));
    return interval_gate_batch(c, c->stage_words(), min, max, nullptr, nullptr, num_bits, 1);
}

pg_status pg_composer_range_gate_batch(pg_composer *c, const pg_variable *d_witness_var, uint64_t num_bits, uint64_t batch) {
    return range_gate_batch(c, d_witness_var, num_bits, batch);
}
pg_status pg_composer_range_gate(pg_composer *c, pg_variable witness, uint64_t num_bits) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(range_num_bits(num_bits));
    PG_TRY(stage_variable(c, witness));
    return range_gate_batch(c, c->stage_words(), num_bits, 1);
}

pg_status pg_composer_is_less_equal_batch(pg_composer *c, const pg_variable *d_x_var, const pg_variable *d_y_var, uint64_t num_bits,
                                          int strict, uint64_t batch, pg_variable *d_result_vars) {
    return is_less_equal_batch(c, d_x_var, d_y_var, num_bits, strict != 0, batch, d_result_vars);
}
pg_status pg_composer_is_less_equal(pg_composer *c, pg_variable x, pg_variable y, uint64_t num_bits, int strict, pg_variable *result) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    if (!result) return fail(PG_ERR_INVALID_ARGUMENT, "is_less_equal: result is NULL");
    PG_TRY(compare_num_bits(num_bits));
    PG_TRY(flush(c));
    PG_TRY(check_var(c, x));
    PG_TRY(check_var(c, y));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    pg::StageBlob b{};
    b.w[0] = x;
    b.w[1] = y;
    PG_TRY(stage(c, b, 2));
    const pg_variable first = c->nvars;  // the item's first new Variable is its result
    PG_TRY(is_less_equal_batch(c, c->stage_words(), c->stage_words() + 1, num_bits, strict != 0, 1, nullptr));
    *result = first;
    return PG_OK;
}

}  // extern "C"

namespace {
// The preflight of a weighted sum: the terms' pass and one pass over seg_off, the coefficients and the constants
// (weighted_sum_check_kernel), which leaves their digest and the first entry of each that violates a precondition.  Nothing has used
// an entry of seg_off as an index before this returns PG_OK.
pg_status check_weighted_sum_arrays(pg_composer *c, const pg_variable *d_term_var, const uint64_t *d_seg_off, const pg_scalar *d_coeff,
                                    const pg_scalar *d_constant, uint64_t terms, uint64_t segments, pg_composer::Sig *vars_dg,
                                    pg_composer::Sig *arrays_dg) {
    pg::Preflight r;
    PG_TRY(preflight(c, 3, r, [&](pg::Preflight *d) {
        digest_vars(c, d_term_var, terms, d, 0);
        hipLaunchKernelGGL(pg::weighted_sum_check_kernel, dim3(grid_cap((terms + pg::kThreads - 1) / pg::kThreads, (uint64_t)c->e->num_cus * 2)),
                           dim3(pg::kThreads), 0, c->stream, d_seg_off, reinterpret_cast<const uint4 *>(d_coeff),
                           reinterpret_cast<const uint4 *>(d_constant), terms, segments, d);
    }));
    const unsigned long long seg = r.call[pg::kWsBadSegment], co = r.call[pg::kWsBadCoeff], k = r.call[pg::kWsBadConstant];
    if (seg != ~0ull)
        return fail(PG_ERR_INVALID_ARGUMENT, "weighted_sum: d_seg_off must start at 0, end at terms = " + std::to_string(terms) +
                                                 " and give every segment at least 2 terms; the first offending segment is " + std::to_string(seg));
    if (co != ~0ull) return fail(PG_ERR_INVALID_ARGUMENT, "weighted_sum: coefficient " + std::to_string(co) + " is not reduced below the modulus");
    if (k != ~0ull) return fail(PG_ERR_INVALID_ARGUMENT, "weighted_sum: constant " + std::to_string(k) + " is not reduced below the modulus");
    *vars_dg = sig_of(r.vars);
    *arrays_dg = sig_of(r.others);
    return PG_OK;
}

// the three launches of weighted_sum.hpp on the composer's stream; one tile: the writer alone
pg_status weighted_sum_launch(pg_composer *c, const pg_variable *d_term_var, const uint64_t *d_seg_off, const pg_scalar *d_coeff,
                              const pg_scalar *d_constant, const pg_scalar *values, uint64_t terms, uint64_t segments,
                              const pg_columns *at, pg_variable *d_result_vars, bool values_only) {
    pg::WeightedSumArgs A{};
    A.term_var = d_term_var;
    A.seg_off = d_seg_off;
    A.val = reinterpret_cast<const uint4 *>(values);
    A.coeff = reinterpret_cast<const uint4 *>(d_coeff);
    A.konst = reinterpret_cast<const uint4 *>(d_constant);
    A.terms = terms;
    A.segments = segments;
    A.tiles = (terms + pg::kWsTile - 1) / pg::kWsTile;
    A.q[0] = reinterpret_cast<uint4 *>(at->q_m);
    A.q[1] = reinterpret_cast<uint4 *>(at->q_l);
    A.q[2] = reinterpret_cast<uint4 *>(at->q_r);
    A.q[3] = reinterpret_cast<uint4 *>(at->q_o);
    A.q[4] = reinterpret_cast<uint4 *>(at->q_c);
    A.w[0] = at->w_l;
    A.w[1] = at->w_r;
    A.w[2] = at->w_o;
    A.vars = reinterpret_cast<uint4 *>(at->var_values);
    A.var_base = c->nvars;
    A.result_vars = d_result_vars;
    if (A.tiles > 1) {
        // per tile: its sum and its carry (32 bytes each), then the flags
        PG_TRY(perm_reserve(c, c->wsum_ws, A.tiles * (2 * sizeof(pg_scalar) + sizeof(uint32_t))));
        A.tile_sum = c->wsum_ws.as<uint4>();
        A.tile_carry = A.tile_sum + 2 * A.tiles;
        A.tile_flag = reinterpret_cast<uint32_t *>(A.tile_carry + 2 * A.tiles);
        hipLaunchKernelGGL(pg::weighted_sum_tiles_kernel, dim3((uint32_t)A.tiles), dim3(pg::kThreads), 0, c->stream, A);
        hipLaunchKernelGGL(pg::weighted_sum_carry_kernel, dim3(1), dim3(pg::kThreads), 0, c->stream, A);
    }
    if (values_only) hipLaunchKernelGGL(pg::weighted_sum_write_kernel<false>, dim3((uint32_t)A.tiles), dim3(pg::kThreads), 0, c->stream, A);
    else hipLaunchKernelGGL(pg::weighted_sum_write_kernel<true>, dim3((uint32_t)A.tiles), dim3(pg::kThreads), 0, c->stream, A);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}
}  // namespace

extern "C" {

pg_status pg_weighted_sum_geometry(uint32_t *tile_terms, uint32_t *tiles_per_carry_pass) {
    if (!tile_terms || !tiles_per_carry_pass) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    *tile_terms = pg::kWsTile;
    *tiles_per_carry_pass = pg::kWsCarryPass;
    return PG_OK;
}

// The rows leave no footprint (sigma and the wire values take the generic routes).  The rows: the four arrays' contents, with NULL
// told from present, terms, segments and where the call lands.
pg_status pg_composer_weighted_sum_ragged_batch(pg_composer *c, const pg_variable *d_term_var, const uint64_t *d_seg_off,
                                                const pg_scalar *d_coeff, const pg_scalar *d_constant, uint64_t terms, uint64_t segments,
                                                pg_variable *d_result_vars) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    if (segments == 0) {
        if (terms) return fail(PG_ERR_INVALID_ARGUMENT, "weighted_sum: " + std::to_string(terms) + " terms in no segment");
        return flush(c);
    }
    if (terms >> 32) return fail(PG_ERR_INVALID_ARGUMENT, "weighted_sum: terms must be below 2^32, got " + std::to_string(terms));
    if (terms == 0)
        return fail(PG_ERR_INVALID_ARGUMENT, "weighted_sum: every segment needs at least 2 terms; the first offending segment is 0");
    PG_TRY(check_u64s(d_seg_off, "d_seg_off"));
    if (d_coeff) PG_TRY(check_scalars(d_coeff, "d_coeff"));
    if (d_constant) PG_TRY(check_scalars(d_constant, "d_constant"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    const uint64_t rows = terms > segments ? terms - segments : 0;  // (terms >= 2 segments once the arrays are checked)
    pg::Fr b0 = pg::fr_zero();  // what the signature has for the arrays: their digest, and which of the optional ones are there
    b0.l[2] = (d_coeff ? 1u : 0u) | (d_constant ? 2u : 0u);
    return var_batch(
        c, {{d_term_var, "d_term_var"}}, terms, rows, rows,
        [&](pg_composer::Sig *dg) -> pg_status {
            pg_composer::Sig arrays;
            PG_TRY(check_weighted_sum_arrays(c, d_term_var, d_seg_off, d_coeff, d_constant, terms, segments, dg, &arrays));
            b0.l[0] = arrays.a;
            b0.l[1] = arrays.b;
            return PG_OK;
        },
        [&](const pg_composer::Sig &dg) { return gadget_sig(c, SigKind::WEIGHTED_SUM_RAGGED_BATCH, b0, pg::fr_zero(), terms, segments, dg); },
        [&](const pg_columns *at, const pg_scalar *values, bool in_place) {
            return weighted_sum_launch(c, d_term_var, d_seg_off, d_coeff, d_constant, values, terms, segments, at, d_result_vars, in_place);
        },
        [] {});
}

pg_status pg_composer_conditionally_select_zero_batch(pg_composer *c, const pg_variable *d_x_var, const pg_variable *d_select_var,
                                                      uint64_t batch, pg_variable *d_result_vars) {
    return two_input_batch<pg::SelectZeroGD>(c, SigKind::SELECT_ZERO_BATCH, pg::WIRES_SELECT_ZERO, d_x_var, d_select_var, batch, d_result_vars);
}
pg_status pg_composer_conditionally_select_one_batch(pg_composer *c, const pg_variable *d_y_var, const pg_variable *d_selector_var,
                                                     uint64_t batch, pg_variable *d_result_vars) {
    return two_input_batch<pg::SelectOneGD>(c, SigKind::SELECT_ONE_BATCH, pg::WIRES_SELECT_ONE, d_y_var, d_selector_var, batch, d_result_vars);
}
pg_status pg_composer_maybe_equal_batch(pg_composer *c, const pg_variable *d_a_var, const pg_variable *d_b_var, uint64_t batch,
                                        pg_variable *d_result_vars) {
    return two_input_batch<pg::MaybeEqualGD>(c, SigKind::MAYBE_EQUAL_BATCH, pg::WIRES_MAYBE_EQUAL, d_a_var, d_b_var, batch, d_result_vars);
}

namespace {
pg_status ragged_alloc(uint64_t batch, bool with_bits, RaggedBuffers *b) {
    if (b->row_off.reserve((batch + 1) * 8) != PG_OK || b->var_off.reserve((batch + 1) * 8) != PG_OK ||
        (with_bits && b->num_bits.reserve(batch * 4) != PG_OK))
        return fail(PG_ERR_HIP, "hipMalloc of the call's prefix sums failed");
    return PG_OK;
}
}  // namespace
}  // extern "C"

namespace {
// The batches whose items differ in shape (per-item public bounds; items that stop at is_non_zero's error, scalar.rs:73-80): the call's
// prefix sums are planned on the device, the rows emitted by them, and the composer keeps them for the f-rows.
//   plan(b, &lay, &errs)  the call's pg_*_plan: row_off / var_off (and the ladder lengths), the totals, the items that fail
//   sign(errs, &sig)      the call's signature
//   emit(b, &at, in_place) its *_common call
// A batch without failing items of a kind whose full items are all alike leaves a uniform footprint.
template <class Plan, class Sign, class Emit>
pg_status ragged_batch(pg_composer *c, uint32_t wire_kind, uint64_t batch, uint64_t *err_count, Plan plan, Sign sign, Emit emit) {
    const bool per_item_bounds = per_item_bounds_kind(wire_kind);
    RaggedBuffers b;
    PG_TRY(ragged_alloc(batch, per_item_bounds, &b));
    pg_layout lay;
    uint64_t errs = 0;
    pg_status st = plan(b, &lay, &errs);
    const bool failed_items = st == PG_ERR_NON_EXISTING_INVERSE;
    if (failed_items) st = PG_OK;
    if (st == PG_OK) st = need(c, lay.n_gates, lay.n_vars);
    pg_composer::Sig sig;
    if (st == PG_OK) st = sign(errs, &sig);
    if (st == PG_OK) {
        const pg_columns at = cols_at(c, c->n, c->nvars);
        SignedAppend sa(c, sig, lay.n_gates);
        st = emit(b, &at, sa.in_place);
        if (st == PG_OK) sa.commit();
    }
    if (st != PG_OK) {  // (the buffers go once nothing reads them any more)
        (void)hipStreamSynchronize(c->stream);
        return st;
    }
    // (per-item bounds: the largest item is the longest ladder there is)
    pg::PermSeg f = pg::footprint(c->n, c->nvars, batch, wire_kind, per_item_bounds ? 255u : 0u);
    if (per_item_bounds || errs) {
        f.gate_end = f.gate_base + lay.n_gates;
        f.var_end = f.var_base + lay.n_vars;
        f.row_off = b.rows();
        f.var_off = b.vars();
        f.wire_n = 0;
    }
    c->ragged.push_back(std::move(b));
    add_footprint(c, f);
    c->n += lay.n_gates;
    c->nvars += lay.n_vars;
    if (err_count) *err_count = errs;
    return failed_items ? fail(PG_ERR_NON_EXISTING_INVERSE, std::to_string(errs) + " item(s) without an inverse") : PG_OK;
}
// an item's shape depends on its witness: only a batch WITHOUT failing items has rows that are a function of public things alone -- a
// batch with one never matches (nor is matched)
uint64_t unmatched_if(pg_composer *c, uint64_t errs) { return errs ? 0x8000000000000000ull | ++c->unmatched : 0; }
}  // namespace

extern "C" {

// the two ladder batches with public bounds per item (WIRES_MAX_BOUND: d_min_range is not looked at).  The rows: the arrays of bounds
// and where the call lands.
static pg_status ragged_ladder_batch(pg_composer *c, uint32_t wire_kind, SigKind kind, const pg_scalar *d_min_range, const pg_scalar *d_max_range,
                                     const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars, uint32_t *d_num_bits_out) {
    const bool with_min = wire_kind == pg::WIRES_RANGE_CHECK;
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));
    if (batch == 0) return PG_OK;
    if (with_min) PG_TRY(check_scalars(d_min_range, "d_min_range"));  // (digested before the engine call that checks the others)
    PG_HIP_TRY(hipSetDevice(c->e->device));
    return ragged_batch(
        c, wire_kind, batch, nullptr,
        [&](RaggedBuffers &b, pg_layout *lay, uint64_t *) {
            return (with_min ? pg_range_check_ragged_plan : pg_max_bound_ragged_plan)(c->e, d_max_range, batch, b.bits(), b.rows(), b.vars(), lay,
                                                                                       c->stream);
        },
        [&](uint64_t, pg_composer::Sig *sig) {
            pg_composer::Sig dg;
            PG_TRY(bounds_digest(c, d_max_range, with_min ? d_min_range : nullptr, batch, &dg));
            *sig = gadget_sig(c, kind, pg::fr_zero(), pg::fr_zero(), batch, 0, dg);
            return PG_OK;
        },
        [&](RaggedBuffers &b, const pg_columns *at, bool in_place) {
            PG_TRY(with_min ? range_check_ragged_common(c->e, d_min_range, d_max_range, d_witness, batch, b.bits(), b.rows(), b.vars(), c->n, c->nvars,
                                                        at, d_result_vars, c->stream, in_place)
                            : max_bound_ragged_common(c->e, d_max_range, d_witness, batch, b.bits(), b.rows(), b.vars(), c->n, c->nvars, at,
                                                      d_result_vars, c->stream, in_place));
            if (d_num_bits_out && hipMemcpyAsync(d_num_bits_out, b.num_bits.get(), batch * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                return fail(PG_ERR_HIP, "copy of the ladder lengths failed");
            return PG_OK;
        });
}
pg_status pg_composer_max_bound_ragged_batch(pg_composer *c, const pg_scalar *d_max_range, const pg_scalar *d_witness,
                                             uint64_t batch, pg_variable *d_result_vars, uint32_t *d_num_bits_out) {
    return ragged_ladder_batch(c, pg::WIRES_MAX_BOUND, SigKind::MAX_BOUND_RAGGED_BATCH, nullptr, d_max_range, d_witness, batch, d_result_vars,
                               d_num_bits_out);
}
pg_status pg_composer_range_check_ragged_batch(pg_composer *c, const pg_scalar *d_min_range, const pg_scalar *d_max_range,
                                               const pg_scalar *d_witness, uint64_t batch, pg_variable *d_result_vars,
                                               uint32_t *d_num_bits_out) {
    return ragged_ladder_batch(c, pg::WIRES_RANGE_CHECK, SigKind::RANGE_CHECK_RAGGED_BATCH, d_min_range, d_max_range, d_witness, batch,
                               d_result_vars, d_num_bits_out);
}

pg_status pg_composer_is_non_zero_batch(pg_composer *c, const pg_variable *d_var, uint64_t batch, uint8_t *d_err_mask,
                                        uint64_t *err_count) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));
    if (err_count) *err_count = 0;
    if (batch == 0) return PG_OK;
    PG_TRY(check_u64s(d_var, "d_var"));
    pg_composer::Sig dg;
    PG_TRY(check_var_arrays(c, {d_var}, batch, &dg));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    PG_TRY(perm_reserve(c, c->val_ws, batch * sizeof(pg_scalar)));
    pg_scalar *const d_vals = c->val_ws.as<pg_scalar>();
    PG_TRY(gather_values(c, d_var, batch, d_vals));
    return ragged_batch(
        c, pg::WIRES_IS_NON_ZERO, batch, err_count,
        [&](RaggedBuffers &b, pg_layout *lay, uint64_t *errs) {
            return pg_is_non_zero_plan(c->e, d_vals, batch, b.rows(), b.vars(), d_err_mask, lay, errs, c->stream);
        },
        [&](uint64_t errs, pg_composer::Sig *sig) {
            *sig = gadget_sig(c, SigKind::IS_NON_ZERO_BATCH, pg::fr_zero(), pg::fr_zero(), batch, unmatched_if(c, errs), dg);
            return PG_OK;
        },
        [&](RaggedBuffers &b, const pg_columns *at, bool in_place) {
            return is_non_zero_common(c->e, d_var, d_vals, batch, b.rows(), b.vars(), c->n, c->nvars, c->zero_var, at, c->stream, in_place);
        });
}

pg_status pg_composer_scalar_mix_batch(pg_composer *c, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                                       const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, pg_variable *d_result_vars,
                                       uint8_t *d_err_mask, uint64_t *err_count) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));
    if (err_count) *err_count = 0;
    if (batch == 0) return PG_OK;
    PG_HIP_TRY(hipSetDevice(c->e->device));
    return ragged_batch(
        c, pg::WIRES_MIX, batch, err_count,
        [&](RaggedBuffers &b, pg_layout *lay, uint64_t *errs) {
            return pg_scalar_mix_plan(c->e, d_v, batch, b.rows(), b.vars(), d_err_mask, lay, errs, c->stream);
        },
        [&](uint64_t errs, pg_composer::Sig *sig) {
            *sig = gadget_sig(c, SigKind::SCALAR_MIX_BATCH, pg::fr_zero(), pg::fr_zero(), batch, unmatched_if(c, errs));
            return PG_OK;
        },
        [&](RaggedBuffers &b, const pg_columns *at, bool in_place) {
            return scalar_mix_common(c->e, d_v, d_y, d_s, d_a, d_b, batch, b.rows(), b.vars(), c->n, c->nvars, c->zero_var, at, d_result_vars,
                                     c->stream, in_place);
        });
}

namespace {
pg_status gate_batch(pg_composer *c, uint32_t op, const pg_variable *d_a, const pg_variable *d_b, const pg_variable *d_c,
                     const pg::Fr &q_m, const pg::Fr &q_l, const pg::Fr &q_r, const pg::Fr &q_o, const pg::Fr &q_c, uint64_t batch,
                     pg_variable *d_out_vars) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));
    if (batch == 0) return PG_OK;
    const bool creates = op == pg::OP_ADD || op == pg::OP_MUL;
    PG_TRY(check_u64s(d_a, "first Variable array"));
    PG_TRY(check_u64s(d_b, "second Variable array"));
    if (!creates) PG_TRY(check_u64s(d_c, "third Variable array"));
    PG_TRY(check_u64s(d_out_vars, "d_out_vars", true));
    for (const pg::Fr *q : {&q_m, &q_l, &q_r, &q_o, &q_c})
        if (!is_reduced(*q)) return fail(PG_ERR_INVALID_ARGUMENT, "selector is not a reduced BlsScalar");
    pg_composer::Sig dg;
    PG_TRY(check_var_arrays(c, {d_a, d_b == d_a ? nullptr : d_b, creates || d_c == d_a ? nullptr : d_c}, batch, &dg));
    PG_TRY(need(c, batch, creates ? batch : 0));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    // the rows: the selectors, the Variable arrays (and which of them are one and the same), where the call lands
    SigHasher h;
    h.u64((uint64_t)SigKind::GATE_BATCH); h.u64(op); h.u64(batch); h.u64((d_b == d_a ? 1 : 0) | (!creates && d_c == d_a ? 2 : 0) | (!creates && d_c == d_b ? 4 : 0));
    h.fr(q_m); h.fr(q_l); h.fr(q_r); h.fr(q_o); h.fr(q_c); h.u64(dg.a); h.u64(dg.b);
    h.u64(c->n); h.u64(c->nvars); h.u64(c->zero_var);
    SignedAppend sa(c, h.done(), batch);
    pg::GateBatch B{};
    B.op = op | (sa.in_place ? pg::OP_ROW_IN_PLACE : 0u); B.gate0 = c->n; B.var0 = c->nvars; B.batch = batch;
    B.a = d_a; B.b = d_b; B.c = creates ? nullptr : d_c; B.out_vars = d_out_vars;
    B.q_m = q_m; B.q_l = q_l; B.q_r = q_r; B.q_o = q_o; B.q_c = q_c;
    const uint64_t want = (batch + pg::kThreads - 1) / pg::kThreads, most = (uint64_t)c->e->num_cus * 32;
    hipLaunchKernelGGL(pg::gate_batch_kernel, dim3((uint32_t)(want < most ? want : most)), dim3(pg::kThreads), 0, c->stream, B, c->cols.view());
    PG_HIP_TRY(hipGetLastError());
    sa.commit();
    // one row per item; add / mul: one Variable, a and b come from outside; the others: three Variables from outside, none created --
    // a footprint for the f-rows only where it pays for the launch it costs there (short runs of rows stay rows of single calls)
    if (creates || batch >= pg::kFootprintMinRows) add_footprint(c, pg::footprint(c->n, c->nvars, batch, creates ? pg::WIRES_GATE_OUT : pg::WIRES_GATE_ROWS));
    c->n += batch;
    if (creates) c->nvars += batch;
    return PG_OK;
}
}  // namespace

pg_status pg_composer_poly_gate_batch(pg_composer *c, const pg_variable *d_a, const pg_variable *d_b, const pg_variable *d_c,
                                      const pg_scalar *q_m, const pg_scalar *q_l, const pg_scalar *q_r, const pg_scalar *q_o,
                                      const pg_scalar *q_c, uint64_t batch) {
    if (!q_m || !q_l || !q_r || !q_o || !q_c) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return gate_batch(c, pg::OP_ROW, d_a, d_b, d_c, to_fr(q_m), to_fr(q_l), to_fr(q_r), to_fr(q_o), to_fr(q_c), batch, nullptr);
}
pg_status pg_composer_add_batch(pg_composer *c, const pg_scalar *q_l, const pg_variable *d_a, const pg_scalar *q_r,
                                const pg_variable *d_b, const pg_scalar *q_c, uint64_t batch, pg_variable *d_out_vars) {
    if (!q_l || !q_r || !q_c) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return gate_batch(c, pg::OP_ADD, d_a, d_b, nullptr, pg::fr_zero(), to_fr(q_l), to_fr(q_r), pg::fr_neg_one(), to_fr(q_c), batch, d_out_vars);
}
pg_status pg_composer_mul_batch(pg_composer *c, const pg_scalar *q_m, const pg_variable *d_a, const pg_variable *d_b,
                                const pg_scalar *q_c, uint64_t batch, pg_variable *d_out_vars) {
    if (!q_m || !q_c) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return gate_batch(c, pg::OP_MUL, d_a, d_b, nullptr, to_fr(q_m), pg::fr_zero(), pg::fr_zero(), pg::fr_neg_one(), to_fr(q_c), batch, d_out_vars);
}
pg_status pg_composer_constrain_to_constant_batch(pg_composer *c, const pg_variable *d_a, const pg_scalar *constant, uint64_t batch) {
    if (!constant) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    // poly_gate(a, a, a, 0, 1, 0, 0, -constant, None)
    return gate_batch(c, pg::OP_ROW, d_a, d_a, d_a, pg::fr_zero(), pg::fr_one(), pg::fr_zero(), pg::fr_zero(), pg::fr_neg(to_fr(constant)),
                      batch, nullptr);
}
pg_status pg_composer_boolean_gate_batch(pg_composer *c, const pg_variable *d_a, uint64_t batch) {
    // (a, a, a; 1, 0, 0, -1, 0)
    return gate_batch(c, pg::OP_ROW, d_a, d_a, d_a, pg::fr_one(), pg::fr_zero(), pg::fr_zero(), pg::fr_neg_one(), pg::fr_zero(), batch, nullptr);
}

pg_status pg_composer_add_input_batch(pg_composer *c, const pg_scalar *d_scalars, uint64_t batch, pg_variable *first_var) {
    if (!c || !first_var) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(flush(c));
    PG_TRY(need(c, 0, batch));
    if (batch) {
        PG_TRY(check_scalars(d_scalars, "d_scalars"));
        PG_HIP_TRY(hipSetDevice(c->e->device));
        PG_HIP_TRY(hipMemcpyAsync(c->cols.view().vars + 2 * c->nvars, d_scalars, batch * 32, hipMemcpyDeviceToDevice, c->stream));
    }
    *first_var = c->nvars;
    c->nvars += batch;
    return PG_OK;
}

pg_status pg_composer_copy_out(pg_composer *c, uint64_t gate_first, uint64_t n_gates, uint64_t var_first, uint64_t n_vars,
                               const pg_columns *dst) {
    if (!c || !dst) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(flush(c));
    if (gate_first + n_gates > c->n || var_first + n_vars > c->nvars) return fail(PG_ERR_INVALID_ARGUMENT, "range past the end");
    PG_HIP_TRY(hipSetDevice(c->e->device));
    const pg_columns src = cols_at(c, gate_first, var_first);
    pg_scalar *const ds[5] = {dst->q_m, dst->q_l, dst->q_r, dst->q_o, dst->q_c};
    const pg_scalar *const ss[5] = {src.q_m, src.q_l, src.q_r, src.q_o, src.q_c};
    for (int i = 0; i < 5; i++)
        if (ds[i] && n_gates) PG_HIP_TRY(hipMemcpyAsync(ds[i], ss[i], n_gates * 32, hipMemcpyDeviceToDevice, c->stream));
    uint64_t *const dw[3] = {dst->w_l, dst->w_r, dst->w_o};
    const uint64_t *const sw[3] = {src.w_l, src.w_r, src.w_o};
    for (int i = 0; i < 3; i++)
        if (dw[i] && n_gates) PG_HIP_TRY(hipMemcpyAsync(dw[i], sw[i], n_gates * 8, hipMemcpyDeviceToDevice, c->stream));
    if (dst->var_values && n_vars)
        PG_HIP_TRY(hipMemcpyAsync(dst->var_values, src.var_values, n_vars * 32, hipMemcpyDeviceToDevice, c->stream));
    return PG_OK;
}

pg_status pg_composer_read_value(pg_composer *c, pg_variable v, pg_scalar *out) {
    if (!c || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(flush(c));
    PG_TRY(check_var(c, v));
    PG_HIP_TRY(hipMemcpyAsync(out, c->cols.view().vars + 2 * v, 32, hipMemcpyDeviceToHost, c->stream));
    PG_HIP_TRY(hipStreamSynchronize(c->stream));
    return PG_OK;
}

// upload the sparse public inputs / fourth-wire rows (small, rare): into device buffers that live as long as B
static pg_status upload_sparse(pg_composer *c, CallBuffers &B, uint64_t **d_gate, uint4 **d_val, pg::FourthWire **d_fw) {
    *d_gate = nullptr; *d_val = nullptr; *d_fw = nullptr;
    const size_t np = c->pi_gate.size(), nf = c->fourth.size();
    if (np) {
        PG_TRY(B.take(d_gate, np * 8));
        PG_TRY(B.take(d_val, np * 32));
        PG_HIP_TRY(hipMemcpyAsync(*d_gate, c->pi_gate.data(), np * 8, hipMemcpyHostToDevice, c->stream));
        PG_HIP_TRY(hipMemcpyAsync(*d_val, c->pi_val.data(), np * 32, hipMemcpyHostToDevice, c->stream));
    }
    if (nf) {
        PG_TRY(B.take(d_fw, nf * sizeof(pg::FourthWire)));
        PG_HIP_TRY(hipMemcpyAsync(*d_fw, c->fourth.data(), nf * sizeof(pg::FourthWire), hipMemcpyHostToDevice, c->stream));
    }
    return PG_OK;
}

pg_status pg_composer_check(pg_composer *c, int64_t *first_bad) {
    if (!c || !first_bad) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(flush(c));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    CallBuffers B(c->stream);
    uint64_t *d_gate; uint4 *d_val; pg::FourthWire *d_fw;
    PG_TRY(upload_sparse(c, B, &d_gate, &d_val, &d_fw));
    unsigned long long *d_bad = nullptr, h_bad = ~0ull;
    PG_TRY(B.take(&d_bad, 8));
    PG_HIP_TRY(hipMemcpyAsync(d_bad, &h_bad, 8, hipMemcpyHostToDevice, c->stream));
    const uint64_t want = (c->n + pg::kThreads - 1) / pg::kThreads;
    const uint32_t grid = (uint32_t)(want < (uint64_t)c->e->num_cus * 8 ? (want ? want : 1) : (uint64_t)c->e->num_cus * 8);
    hipLaunchKernelGGL(pg::check_kernel, dim3(grid), dim3(pg::kThreads), 0, c->stream, c->cols.view(), c->n, (uint64_t)0, c->nvars,
                       c->zero_var, d_gate, d_val, (uint32_t)c->pi_gate.size(), d_fw, (uint32_t)c->fourth.size(), d_bad);
    // the range widget's rows: the minimum over both kinds of failure
    for (const pg::RangeSeg &s : c->range_segs) {
        const uint64_t rw = (s.items * s.g + pg::kThreads - 1) / pg::kThreads, most = (uint64_t)c->e->num_cus * 8;
        hipLaunchKernelGGL(pg::range_check_rows_kernel, dim3((uint32_t)(rw < most ? rw : most)), dim3(pg::kThreads), 0, c->stream, c->cols.view(), s,
                           c->nvars, d_bad);
    }
    PG_HIP_TRY(hipGetLastError());
    PG_HIP_TRY(hipMemcpyAsync(&h_bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    PG_HIP_TRY(hipStreamSynchronize(c->stream));
    *first_bad = h_bad == ~0ull ? -1 : (int64_t)h_bad;
    return PG_OK;
}

pg_status pg_composer_dense_pi(pg_composer *c, pg_scalar *d_out) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));
    PG_TRY(check_scalars(d_out, "d_out"));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    PG_HIP_TRY(hipMemsetAsync(d_out, 0, c->n * 32, c->stream));
    CallBuffers B(c->stream);
    uint64_t *d_gate; uint4 *d_val; pg::FourthWire *d_fw;
    PG_TRY(upload_sparse(c, B, &d_gate, &d_val, &d_fw));
    const uint32_t np = (uint32_t)c->pi_gate.size();
    if (np) {
        hipLaunchKernelGGL(pg::scatter_pi_kernel, dim3((np + 255) / 256), dim3(256), 0, c->stream,
                           reinterpret_cast<uint4 *>(d_out), d_gate, d_val, np);
        PG_HIP_TRY(hipGetLastError());
    }
    PG_HIP_TRY(hipStreamSynchronize(c->stream));
    return PG_OK;
}

pg_status pg_composer_materialize(pg_composer *c, const pg_full_columns *out) {
    if (!c || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(flush(c));
    PG_HIP_TRY(hipSetDevice(c->e->device));
    const uint32_t grid = (uint32_t)c->e->num_cus * 32;
    // q_arith = 1, the other selectors = 0, and the value of the fourth wire = value of zero_var = 0, on every row (the few
    // rows with a live fourth wire are patched afterwards); the wire-value columns gathered by wire index: one launch
    pg::MaterializeOut M{};
    pg_scalar *const consts[7] = {out->q_4, out->q_arith, out->q_range, out->q_logic, out->q_fixed_group_add,
                                  out->q_variable_group_add, out->w_4_value};
    for (int k = 0; k < 7; k++) {
        if (!consts[k]) continue;
        PG_TRY(check_scalars(consts[k], "constant column"));
        M.konst[k] = reinterpret_cast<uint4 *>(consts[k]);
    }
    pg_scalar *const vals[3] = {out->w_l_value, out->w_r_value, out->w_o_value};
    for (int i = 0; i < 3; i++) {
        if (!vals[i]) continue;
        PG_TRY(check_scalars(vals[i], "wire value column"));
        M.val[i] = reinterpret_cast<uint4 *>(vals[i]);
    }
    if (out->w_4) {
        PG_TRY(check_u64s(out->w_4, "w_4"));
        M.w_4 = out->w_4;
    }
    // the rows of batched calls: their items' own Variables from an LDS window read linearly (materialize.hpp); the rows of
    // single calls in between (and calls too small to bother, or whose items outgrow the window): gathered by wire index
    const auto generic = [&](uint64_t lo, uint64_t hi) {
        if (hi <= lo) return;
        const uint64_t want = (2 * (hi - lo) + 16383) / 16384;
        hipLaunchKernelGGL(pg::materialize_kernel, dim3((uint32_t)(want < grid ? want : grid)), dim3(pg::kThreads), 0, c->stream, c->cols.view(), M,
                           lo, hi, c->zero_var);
    };
    uint64_t at = 0;
#ifndef PG_MAT_GRID_PER_CU
#define PG_MAT_GRID_PER_CU 64
#endif
    // materialize_items_kernel's instantiations: MAT_SELF's two ragged forms, MAT_READ_WIRES for any footprint, MAT_SELF by uniform kind
    using MatKernel = void (*)(const pg::ComposerCols, const pg::MaterializeOut, const pg::PermSeg, uint32_t, uint64_t);
    static const MatKernel self_ragged[2] = {pg::materialize_items_kernel<pg::MAT_SELF, pg::WIRES_MAX_BOUND, true>,
                                             pg::materialize_items_kernel<pg::MAT_SELF, pg::WIRES_MIX, true>};
    static const MatKernel read_wires = pg::materialize_items_kernel<pg::MAT_READ_WIRES, pg::WIRES_UNKNOWN>;
    static const MatKernel self[pg::WIRES_MIX + 1] = {
        nullptr,
        pg::materialize_items_kernel<pg::MAT_SELF, pg::WIRES_RANGE_CHECK>,
        pg::materialize_items_kernel<pg::MAT_SELF, pg::WIRES_MAX_BOUND>,
        pg::materialize_items_kernel<pg::MAT_SELF, pg::WIRES_RANGE_CHECK_ALLOCATED>,
        pg::materialize_items_kernel<pg::MAT_SELF, pg::WIRES_MAX_BOUND_ALLOCATED>,
        pg::materialize_items_kernel<pg::MAT_SELF, pg::WIRES_DECOMPOSITION>,
        pg::materialize_items_kernel<pg::MAT_SELF, pg::WIRES_MIX>,
    };
    for (const pg::PermSeg &s : c->segs) {
        const uint64_t group = pg::mat_group(s);
        const pg::MatRoute r = pg::mat_route(s, group);
        if (!r.windowed) continue;  // (left to the generic launch of the gap it widens)
        generic(at, s.gate_base);
        const uint64_t n_groups = (s.items + group - 1) / group, most = (uint64_t)c->e->num_cus * PG_MAT_GRID_PER_CU;
        const MatKernel kernel = r.mode != pg::MAT_SELF ? read_wires : r.ragged ? self_ragged[r.kind == pg::WIRES_MIX] : self[r.kind];
        hipLaunchKernelGGL(kernel, dim3((uint32_t)(n_groups < most ? n_groups : most)), dim3(pg::kMatThreads), 0, c->stream, c->cols.view(), M, s,
                           (uint32_t)group, c->zero_var);
        at = s.gate_end;
    }
    generic(at, c->n);
    CallBuffers B(c->stream);
    uint64_t *d_gate; uint4 *d_val; pg::FourthWire *d_fw;
    PG_TRY(upload_sparse(c, B, &d_gate, &d_val, &d_fw));
    if (d_fw)
        hipLaunchKernelGGL(pg::patch_fourth_kernel, dim3(1), dim3(64), 0, c->stream, reinterpret_cast<uint4 *>(out->q_4), out->w_4,
                           reinterpret_cast<uint4 *>(out->w_4_value), c->cols.view().vars, d_fw, (uint32_t)c->fourth.size());
    if (out->q_range)  // the range widget's rows, over the zeros of the passes above
        for (const pg::RangeSeg &s : c->range_segs) {
            const uint64_t rw = (2 * s.items * s.g + pg::kThreads - 1) / pg::kThreads;
            hipLaunchKernelGGL(pg::range_patch_kernel, dim3((uint32_t)(rw < grid ? rw : grid)), dim3(pg::kThreads), 0, c->stream,
                               reinterpret_cast<uint4 *>(out->q_range), s);
        }
    PG_HIP_TRY(hipGetLastError());
    PG_HIP_TRY(hipStreamSynchronize(c->stream));
    return PG_OK;
}

// grows one of the composer's buffers once the stream has drained: work in flight may still read what is there
static pg_status perm_reserve(pg_composer *c, Scratch &buf, size_t bytes) {
    if (bytes <= buf.size()) return PG_OK;
    PG_HIP_TRY(hipStreamSynchronize(c->stream));
    return buf.reserve(bytes);
}

pg_status pg_composer_permutation_reserve(pg_composer *c, uint64_t sparse_positions) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    c->sparse_cap_first = sparse_positions;
    if (sparse_positions) c->perm_last_sparse = 0;  // the caller's figure is used as given (too small: the pass runs twice)
    return PG_OK;
}

// the sigma kernels that ask for more dynamic LDS than the default limit: said once per engine (its device is current)
static pg_status perm_kernel_attributes(pg_engine *e) {
    if (e->perm_attributes_set) return PG_OK;
    const void *const ladder_lds[4] = {
        reinterpret_cast<const void *>(pg::perm_ladder_kernel<false>), reinterpret_cast<const void *>(pg::perm_template_kernel<true>),
        reinterpret_cast<const void *>(pg::perm_template_kernel<false>), reinterpret_cast<const void *>(pg::perm_ladder_kernel<true>)};
    if (pg::kPermLadderLds)
        for (const void *k : ladder_lds) PG_HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pg::kPermLadderLds));
    PG_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pg::perm_identity_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)pg::kPermIdentityLds));
    e->perm_attributes_set = true;
    return PG_OK;
}

pg_status pg_composer_permutation(pg_composer *c, uint64_t padded_n, uint64_t *d_sigma) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "composer is NULL");
    PG_TRY(flush(c));
    PG_TRY(check_u64s(d_sigma, "d_sigma"));
    if (padded_n < c->n) return fail(PG_ERR_INVALID_ARGUMENT, "padded_n is smaller than the circuit");
    PG_HIP_TRY(hipSetDevice(c->e->device));
    PG_TRY(perm_kernel_attributes(c->e));
    const uint32_t grid = (uint32_t)c->e->num_cus * 32;
    uint32_t pos_bits = 2, var_bits = 1;
    while ((1ull << pos_bits) < 4 * c->n) pos_bits++;
    while ((1ull << var_bits) < c->nvars + 1) var_bits++;  // (one number more than there are Variables: the holes' key)
    if (pos_bits + var_bits > 64) return fail(PG_ERR_INVALID_ARGUMENT, "circuit too large for 64-bit (Variable, position) keys");
    // every footprint is classified ONCE (footprint.hpp, perm_route) and each loop below switches on that; a footprint of which not even
    // one item fits a workgroup's LDS is dropped: its rows count as rows of single calls
    std::vector<pg::PermSeg> segs;
    std::vector<pg::PermRoute> routes;
    std::vector<std::pair<uint64_t, uint64_t>> gaps;
    uint64_t at = 0, gap_rows = 0;
    for (pg::PermSeg s : c->segs) {
        const pg::PermRoute route = pg::perm_route(s);
        if (!(s.group = pg::perm_group(s, route))) continue;
        if (s.gate_base > at) gaps.emplace_back(at, s.gate_base);
        segs.push_back(s);
        routes.push_back(route);
        at = s.gate_end;
    }
    if (c->n > at) gaps.emplace_back(at, c->n);
    for (const auto &g : gaps) gap_rows += g.second - g.first;
    const size_t seg_bytes = round256(segs.size() * sizeof(pg::PermSeg));
    const size_t fw_bytes = round256(c->fourth.size() * sizeof(pg::FourthWire));
    PG_TRY(perm_reserve(c, c->perm_small, seg_bytes + fw_bytes + 256));
    char *small = c->perm_small.as<char>();
    pg::PermCtx X;
    X.C = c->cols.view(); X.n = c->n; X.padded_n = padded_n; X.zero_var = c->zero_var;
    X.segs = reinterpret_cast<const pg::PermSeg *>(small); X.n_segs = (uint32_t)segs.size();
    X.fw = reinterpret_cast<const pg::FourthWire *>(small + seg_bytes); X.n_fw = (uint32_t)c->fourth.size();
    X.fw_lo = 0; X.fw_span = 0; X.pos_bits = pos_bits;
    X.hole_key = pos_bits + var_bits >= 64 ? ~0ull : (1ull << (pos_bits + var_bits)) - 1;
    if (!c->fourth.empty()) {
        uint64_t lo = ~0ull, hi = 0;
        for (const pg::FourthWire &f : c->fourth) { lo = f.gate < lo ? f.gate : lo; hi = f.gate > hi ? f.gate : hi; }
        X.fw_lo = lo; X.fw_span = hi - lo;
    }
    // the closed-form routes' slots on the sparse list, ahead of what the other kernels reserve by counter; for the ragged ones the
    // first item of every piece of rows, looked up once per call (perm_piece_items_kernel)
    uint64_t reserved = 0, total_pieces = 0;
    for (size_t i = 0; i < segs.size(); i++) {
        if (pg::perm_reserves_slots(routes[i])) {
            segs[i].sparse_base = reserved;
            reserved += segs[i].items * pg::perm_slots_per_item(segs[i], routes[i]);
        }
        if (pg::perm_needs_piece_items(routes[i])) total_pieces += pg::perm_pieces(segs[i]);
    }
    if (total_pieces) {
        PG_TRY(perm_reserve(c, c->perm_pieces, total_pieces * sizeof(uint32_t)));
        uint32_t *at_piece = c->perm_pieces.as<uint32_t>();
        for (size_t i = 0; i < segs.size(); i++) {
            if (!pg::perm_needs_piece_items(routes[i])) continue;
            pg::PermSeg &s = segs[i];
            s.piece_item = at_piece;
            at_piece += pg::perm_pieces(s);
            const uint64_t want = (s.items + pg::kThreads - 1) / pg::kThreads;
            hipLaunchKernelGGL(pg::perm_piece_items_kernel, dim3((uint32_t)(want < grid ? want : grid)), dim3(pg::kThreads), 0, c->stream, s,
                               pg::kPermLadderRows, at_piece - pg::perm_pieces(s));
        }
        PG_HIP_TRY(hipGetLastError());
    }
    unsigned long long *d_count = reinterpret_cast<unsigned long long *>(small + seg_bytes + fw_bytes);
    // the uploads read host vectors that must outlive them: the synchronisation below covers both
    if (!segs.empty())
        PG_HIP_TRY(hipMemcpyAsync(small, segs.data(), segs.size() * sizeof(pg::PermSeg), hipMemcpyHostToDevice, c->stream));
    if (!c->fourth.empty())
        PG_HIP_TRY(hipMemcpyAsync(small + seg_bytes, c->fourth.data(), c->fourth.size() * sizeof(pg::FourthWire),
                                  hipMemcpyHostToDevice, c->stream));
    // sparse list: every position of the gap rows can land there, those of the items as far as the batched calls said
    // they reference older Variables -- if the list is outgrown the pass reports how long it is and runs once more
    // first-pass size of the list: the caller's (pg_composer_permutation_reserve), else an estimate
    uint64_t cap = c->sparse_cap_first ? c->sparse_cap_first : 4 * gap_rows + c->sparse_hint + (1ull << 16), nS = 0;
    if (cap < c->perm_last_sparse) cap = c->perm_last_sparse;
    uint64_t *k0 = nullptr, *k1 = nullptr, holes = 0;
    size_t tmp_bytes = 0;
    for (int attempt = 0;; attempt++) {
        uint64_t *nul = nullptr;
        PG_HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_bytes, nul, nul, (size_t)cap, 0u, pos_bits + var_bits, c->stream));
        const size_t kb = round256(cap * 8);
        PG_TRY(perm_reserve(c, c->perm_big, 2 * kb + tmp_bytes + 256));
        k0 = c->perm_big.as<uint64_t>();
        k1 = reinterpret_cast<uint64_t *>(c->perm_big.as<char>() + kb);
        const pg::PermSparse Q{k0, d_count, cap};
        hipLaunchKernelGGL(pg::perm_count_init_kernel, dim3(1), dim3(1), 0, c->stream, d_count, reserved);
        for (size_t i = 0; i < segs.size(); i++) {
            const pg::PermSeg &s = segs[i];
            const uint64_t most = (uint64_t)c->e->num_cus * 64, pieces = pg::perm_pieces(s);
            const uint32_t lds = pg::perm_lds_bytes(s, routes[i]);
            // (the closed forms: short pieces, one per workgroup, in dispatch order)
            if (routes[i] != pg::PERM_ITEMS && routes[i] != pg::PERM_LADDER && pieces > 0x7fffffffull)
                return fail(PG_ERR_INVALID_ARGUMENT, "segment too large for one launch");
            switch (routes[i]) {
            case pg::PERM_LADDER: {
                const uint64_t lmost = pg::kPermLadderRows <= 2048 ? 0x7fffffffull : most;
                hipLaunchKernelGGL(pg::perm_ladder_kernel<false>, dim3((uint32_t)(pieces < lmost ? pieces : lmost)), dim3(pg::kThreads), lds,
                                   c->stream, X, s, Q, d_sigma);
                break;
            }
            case pg::PERM_LADDER_RAGGED:
                hipLaunchKernelGGL(pg::perm_ladder_kernel<true>, dim3((uint32_t)pieces), dim3(pg::kThreads), lds, c->stream, X, s, Q, d_sigma);
                break;
            case pg::PERM_TEMPLATE:
                hipLaunchKernelGGL(pg::perm_template_kernel<false>, dim3((uint32_t)pieces), dim3(pg::kThreads), lds, c->stream, X, s,
                                   pg::template_rows(s.wire_kind), Q, d_sigma);
                break;
            case pg::PERM_TEMPLATE_RAGGED:
                hipLaunchKernelGGL(pg::perm_template_kernel<true>, dim3((uint32_t)pieces), dim3(pg::kThreads), lds, c->stream, X, s,
                                   pg::template_rows(s.wire_kind), Q, d_sigma);
                break;
            case pg::PERM_ITEMS: {
                const uint64_t groups = (s.items + s.group - 1) / s.group;
                hipLaunchKernelGGL(pg::perm_item_kernel, dim3((uint32_t)(groups < most ? groups : most)), dim3(pg::kThreads), lds, c->stream, X, s,
                                   groups, Q, d_sigma);
                break;
            }
            }
        }
        for (const auto &g : gaps) {
            const uint64_t nblk = (g.second - g.first + pg::kPermChunk - 1) / pg::kPermChunk;
            hipLaunchKernelGGL(pg::perm_gap_kernel, dim3((uint32_t)nblk), dim3(pg::kThreads), 0, c->stream, X, g.first, g.second, Q,
                               d_sigma);
        }
        PG_HIP_TRY(hipMemcpyAsync(c->totals(), d_count, 16, hipMemcpyDeviceToHost, c->stream));
        PG_HIP_TRY(hipStreamSynchronize(c->stream));
        nS = c->totals()[0];
        holes = c->totals()[1];
        c->perm_last_sparse = nS;
        if (nS <= cap) break;
        if (attempt) return fail(PG_ERR_HIP, "sparse position list grew between two passes");
        cap = nS;
    }
    if (nS) {
        PG_HIP_TRY(rocprim::radix_sort_keys(c->perm_big.as<char>() + 2 * round256(cap * 8), tmp_bytes, k0, k1,
                                            (size_t)nS, 0u, pos_bits + var_bits, c->stream));
        nS -= holes;  // (sorted to the end: reserved slots of ladder items whose witness is zero_var -- the zero chain has those positions)
    }
    if (nS) {
        const uint64_t want = (nS + pg::kThreads - 1) / pg::kThreads;
        hipLaunchKernelGGL(pg::perm_sparse_link_kernel, dim3((uint32_t)(want < grid ? want : grid)), dim3(pg::kThreads), 0, c->stream,
                           X, k1, nS, d_sigma);
        if (!segs.empty()) {
            const uint64_t wantw = (nS + 255) / 256;
            hipLaunchKernelGGL(pg::perm_splice_kernel, dim3((uint32_t)(wantw < grid ? wantw : grid)), dim3(pg::kThreads), 0, c->stream,
                               X, k1, nS, d_sigma);
        }
    }
    if (padded_n > c->n) {
        // (every run is padded_n - n entries, give or take the odd one at either end: the same number of workgroups for each)
        const uint64_t per_run = ((padded_n - c->n) / 2 + 1 + pg::kPermIdentityUnits - 1) / pg::kPermIdentityUnits;
        if (4 * per_run > 0x7fffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "padding too large for one launch");
        hipLaunchKernelGGL(pg::perm_identity_kernel, dim3((uint32_t)(4 * per_run)), dim3(pg::kThreads), pg::kPermIdentityLds, c->stream,
                           d_sigma, c->n, padded_n);
    }
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_check_rows(pg_engine *e, const pg_columns *cols, uint64_t n_gates, uint64_t var_base, uint64_t n_vars,
                        pg_variable zero_var, int64_t *first_bad, void *stream) {
    if (!e || !first_bad) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    *first_bad = -1;
    if (n_gates == 0) return PG_OK;
    PG_TRY(check_columns(cols));
    PG_HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    pg::ComposerCols C;
    C.q[0] = reinterpret_cast<uint4 *>(cols->q_m); C.q[1] = reinterpret_cast<uint4 *>(cols->q_l);
    C.q[2] = reinterpret_cast<uint4 *>(cols->q_r); C.q[3] = reinterpret_cast<uint4 *>(cols->q_o);
    C.q[4] = reinterpret_cast<uint4 *>(cols->q_c);
    C.w[0] = cols->w_l; C.w[1] = cols->w_r; C.w[2] = cols->w_o;
    C.vars = reinterpret_cast<uint4 *>(cols->var_values);
    unsigned long long *d_bad = nullptr, h_bad = ~0ull;
    CallBuffers B(st);
    PG_TRY(B.take(&d_bad, 8));
    PG_HIP_TRY(hipMemcpyAsync(d_bad, &h_bad, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pg::check_kernel, dim3((uint32_t)e->num_cus * 16), dim3(pg::kThreads), 0, st, C, n_gates, var_base, n_vars,
                       zero_var, (const uint64_t *)nullptr, (const uint4 *)nullptr, 0u, (const pg::FourthWire *)nullptr, 0u, d_bad);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) le = hipMemcpyAsync(&h_bad, d_bad, 8, hipMemcpyDeviceToHost, st);
    if (le == hipSuccess) le = hipStreamSynchronize(st);
    if (le != hipSuccess) return fail(PG_ERR_HIP, std::string("pg_check_rows: ") + hipGetErrorString(le));
    *first_bad = h_bad == ~0ull ? -1 : (int64_t)h_bad;
    return PG_OK;
}

}  // extern "C"
