// capi.hip -- the C ABI of libplonk_gadgets_hip.so (include/plonk_gadgets_hip.h).
// Host-side validation and layout arithmetic + kernel launches.  There is no
// CPU fallback anywhere in this file: a call either runs on the GPU or
// returns an error status.
#include "../../include/plonk_gadgets_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>
#include <functional>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "emit.hpp"
#include "fr.hpp"
#include "range_gadgets.hpp"
#include "range_gate.hpp"
#include "scalar_gadgets.hpp"
#include "composer.hpp"
#include "interval_gate.hpp"
#include "compare_gate.hpp"
#include "weighted_sum.hpp"
#include "permutation.hpp"
#include "materialize.hpp"
#include "permutation_product.hpp"
#include "ntt.hpp"
#include "quotient.hpp"
#include "host_util.hpp"

#ifndef PG_GRID_BLOCKS_PER_CU
// more workgroups than can be resident: the dispatcher back-fills CUs as tiles finish (+6 % over a persistent
// 8-per-CU grid on the C2 shape, tools/ab_emit.py)
#define PG_GRID_BLOCKS_PER_CU 64
#endif
#ifndef PG_EMIT_GRID_BLOCKS_PER_CU
// the full emission of a big-item gadget: at most this many tiles' worth of workgroups, i.e. ONE tile per workgroup, in dispatch order,
// up to 2^20 items of C4's shape (65536 tiles; with 64 per CU a workgroup walked four tiles 16384 apart): 17.45 -> 17.07 ms and
// 18.34 -> 17.90 on two boxes; C2's shape (32768 tiles) 33.31 / 33.27, C3's unchanged.  The witness refresh keeps 64: one tile per
// workgroup costs it 5.6 -> 6.15 ms on the tables that are fast (tools/ab_emit.py run_values, `ga`)
#define PG_EMIT_GRID_BLOCKS_PER_CU 256
#endif

namespace {

pg_status check_columns(const pg_columns *c) {
    if (!c) return fail(PG_ERR_INVALID_ARGUMENT, "columns is NULL");
    const void *sc[6] = {c->q_m, c->q_l, c->q_r, c->q_o, c->q_c, c->var_values};
    for (const void *p : sc)
        if (!p || !aligned(p, 16)) return fail(PG_ERR_INVALID_ARGUMENT, "scalar column NULL or not 16-byte aligned");
    const void *wc[3] = {c->w_l, c->w_r, c->w_o};
    for (const void *p : wc)
        if (!p || !aligned(p, 8)) return fail(PG_ERR_INVALID_ARGUMENT, "wire column NULL or not 8-byte aligned");
    return PG_OK;
}

}  // namespace

struct pg_engine {
    int device = -1;
    int num_cus = 0;
    // Every member below that owns something (owners.hpp) is released by its destructor: delete e in pg_engine_destroy, which
    // first makes the engine's device current and drains the side stream and the last copy out of `seg`.  After that no member
    // depends on another, so their order says nothing about release.
    Scratch d_pow2;  // mont(2^i), i < 256
    // scratch of the ragged plans: per-item counts (uint32_t), block sums (uint64_t), error counter (uint32_t)
    Scratch d_rows, d_vars, d_blk_rows, d_blk_vars;
    Scratch d_blk_agg;  // single-launch plans (emit.hpp, PlanScan): published block totals (unsigned long long); [blocks] = blocks done
    Scratch d_err_count;
    uint64_t scratch_items = 0, scratch_blocks = 0;
    // totals of the last plan, written by async copies into pinned host memory (read after a synchronisation)
    using PlanResult = pg::PlanTotals;
    Pinned h_plan;
    PlanResult *plan() const { return h_plan.as<PlanResult>(); }
    // behind it in the same pinned block, the bulk decoder's count of bad encodings: a word of its own, so that a decode between an
    // asynchronous plan and pg_plan_result leaves the plan's totals alone
    uint32_t *bad_encodings() const { return reinterpret_cast<uint32_t *>(h_plan.as<PlanResult>() + 1); }
    // scratch of the inversions: the pre-pass parks an element and its running product (64 B per element),
    // the fused mix one running product per item (32 B)
    Scratch d_prefix;
    uint64_t inv_elems = 0;
    // the pre-pass runs on its own stream beside the rows-only emit launch
    Stream side;
    Event ev_fork, ev_inv;
    // the stream the last call was issued on (see enter_stream)
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    Event ev_switch;
    // scratch of pg_sigma_evaluations / pg_permutation_product: flags, omega tables, tile products, denominators
    Scratch d_pp;
    // scratch of pg_ntt: its omega and coset tables
    Scratch d_ntt;
    // scratch of pg_quotient: its table of the chunk's points x; of pg_poly_evaluate: its power tables and partial sums
    Scratch d_quot, d_eval;
    // scratch of pg_msm (sort keys, partial and bucket sums) and of pg_srs_setup (fixed-base tables, a chunk of points)
    Scratch d_msm, d_srs;
    // scratch of pg_msm_segmented: products, sums and segment offsets; the pinned buffer its offsets are staged in
    Scratch d_msm_small;
    Staging seg;
    // scratch of pg_poly_open: its tile totals and carries
    Scratch d_open;
    // scratch of pg_plonk_sides: the decode status of every commitment, 11 bytes a proof
    Scratch d_sides;
    // pg_composer_permutation: its kernels' dynamic LDS limits have been raised on this device (capi_composer.inc, perm_kernel_attributes)
    bool perm_attributes_set = false;
};

namespace {

pg_status ensure_scratch(pg_engine *e, uint64_t batch) {
    if (batch <= e->scratch_items && e->d_err_count.get()) return PG_OK;
    PG_HIP_TRY(hipSetDevice(e->device));
    e->scratch_items = 0;
    const uint64_t items = batch < 1024 ? 1024 : batch;
    // (the published words: one per block of a plan kernel, or per wave of the fused mix's planning launch -- at most 2048
    // of those up to 2 M items, one per 1024 items beyond)
    const uint64_t nblk = std::max<uint64_t>((items + pg::kScanBlock - 1) / pg::kScanBlock, 2048);
    PG_TRY(e->d_rows.reserve(items * sizeof(uint32_t)));
    PG_TRY(e->d_vars.reserve(items * sizeof(uint32_t)));
    PG_TRY(e->d_blk_rows.reserve(nblk * sizeof(uint64_t)));
    PG_TRY(e->d_blk_vars.reserve(nblk * sizeof(uint64_t)));
    PG_TRY(e->d_blk_agg.reserve((nblk + 1) * sizeof(unsigned long long)));
    PG_HIP_TRY(hipMemset(e->d_blk_agg.get(), 0, (nblk + 1) * sizeof(unsigned long long)));  // zero between launches: the plan kernels leave them so
    e->scratch_blocks = nblk;
    if (!e->d_err_count.get()) {
        PG_TRY(e->d_err_count.reserve(sizeof(uint32_t)));
        PG_HIP_TRY(hipMemset(e->d_err_count.get(), 0, sizeof(uint32_t)));  // zero between calls (see error_plan)
    }
    e->scratch_items = items;
    return PG_OK;
}

// what a plan kernel is handed to finish the prefix sums itself (up to kPlanFusedBlocks blocks; beyond, fused = 0 and
// scan_counts launches the two-level scan)
pg::PlanScan plan_scan(pg_engine *e, uint64_t batch, uint64_t *d_row_off, uint64_t *d_var_off, bool with_errs,
                       uint32_t fused_blocks = pg::kPlanFusedBlocks) {
    const uint64_t nblk = (batch + pg::kScanBlock - 1) / pg::kScanBlock;
    pg::PlanScan P{};
    P.agg = e->d_blk_agg.as<unsigned long long>();
    P.blocks_cap = (uint32_t)e->scratch_blocks;
    P.blk_rows = e->d_blk_rows.as<uint64_t>();
    P.blk_vars = e->d_blk_vars.as<uint64_t>();
    P.row_off = d_row_off;
    P.var_off = d_var_off;
    P.host = e->plan();
    P.err_count = with_errs ? e->d_err_count.as<uint32_t>() : nullptr;
#if defined(PG_PLAN_TWO_LAUNCHES)  // A/B build
    P.fused = 0;
#else
    P.fused = nblk <= fused_blocks ? 1u : 0u;
#endif
    return P;
}

pg_status plan_totals(pg_engine *e, uint64_t *n_rows, uint64_t *n_vars) {
    if (e->plan()->pad) {
        e->plan()->pad = 0;
        return fail(PG_ERR_HIP, "a plan's look-back gave up waiting for another block's totals");
    }
    *n_rows = e->plan()->n_gates;
    *n_vars = e->plan()->n_vars;
    return PG_OK;
}

// counts in e->d_rows / e->d_vars and their block sums in e->d_blk_* (both left by the plan kernel) -> exclusive prefix
// sums; totals copied back (the synchronous form synchronises the stream).  Nothing to launch after a fused plan.
pg_status scan_counts(pg_engine *e, uint64_t batch, uint64_t *d_row_off, uint64_t *d_var_off, uint64_t *n_rows,
                      uint64_t *n_vars, hipStream_t st, bool with_errs, uint32_t fused_blocks = pg::kPlanFusedBlocks) {
    const uint32_t nblk = (uint32_t)((batch + pg::kScanBlock - 1) / pg::kScanBlock);
    if (!plan_scan(e, batch, d_row_off, d_var_off, with_errs, fused_blocks).fused) {
        const uint32_t prefixed = nblk > pg::kScanDirectBlocks ? 1u : 0u;
        if (prefixed)
            hipLaunchKernelGGL(pg::scan_top_kernel, dim3(1), dim3(pg::kThreads), 0, st, e->d_blk_rows.as<uint64_t>(),
                               e->d_blk_vars.as<uint64_t>(), nblk);
        hipLaunchKernelGGL(pg::scan_final_kernel, dim3(nblk), dim3(pg::kThreads), 0, st, e->d_rows.as<uint32_t>(),
                           e->d_vars.as<uint32_t>(), batch, e->d_blk_rows.as<uint64_t>(), e->d_blk_vars.as<uint64_t>(), d_row_off,
                           d_var_off, prefixed, e->plan(), with_errs ? e->d_err_count.as<uint32_t>() : nullptr);
        PG_HIP_TRY(hipGetLastError());
    }
    if (n_rows) {  // synchronous form
        PG_HIP_TRY(hipStreamSynchronize(st));
        PG_TRY(plan_totals(e, n_rows, n_vars));
    }
    return PG_OK;
}

pg::EmitOut make_out(const pg_columns *c, uint64_t batch, int W, uint64_t gate_base, uint64_t var_base, uint64_t zero_var,
                     const uint64_t *row_off, const uint64_t *var_off) {
    pg::EmitOut O;
    O.q[0] = reinterpret_cast<uint4 *>(c->q_m);
    O.q[1] = reinterpret_cast<uint4 *>(c->q_l);
    O.q[2] = reinterpret_cast<uint4 *>(c->q_r);
    O.q[3] = reinterpret_cast<uint4 *>(c->q_o);
    O.q[4] = reinterpret_cast<uint4 *>(c->q_c);
    O.w[0] = c->w_l;
    O.w[1] = c->w_r;
    O.w[2] = c->w_o;
    O.vars = reinterpret_cast<uint4 *>(c->var_values);
    O.gate_base = gate_base;
    O.var_base = var_base;
    O.zero_var = zero_var;
    O.row_off = row_off;
    O.var_off = var_off;
    O.batch = batch;
    O.tiles = (uint32_t)((batch + W - 1) / W);
    O.stride_rows = 0;
    O.inv_dense = nullptr;
    O.inv_elems = 0;
    O.inv_in_place = 1;
    O.early_span = O.early_tiles = 0;
    return O;
}

pg_status ensure_inv_scratch(pg_engine *e, uint64_t elems) {
    if (elems <= e->inv_elems) return PG_OK;
    PG_HIP_TRY(hipSetDevice(e->device));
    e->inv_elems = 0;
    // per element: the element and its running product; + 64 x 16 bytes that the fused mix's masked lanes store to
    PG_TRY(e->d_prefix.reserve((elems * 4 + 64 + 4 * 32 * 32 * 8) * sizeof(uint4)));  // (+ the fused mix's last workgroup: whole steps of whole waves)
    e->inv_elems = elems;
    return PG_OK;
}

// the engine's events order streams of ONE device against each other and are never waited for by the host: without the
// system-scope fence a default event performs when it completes (cache write-back and invalidation: microseconds on the
// stream, after every call)
constexpr unsigned kOrderingEvent = hipEventDisableTiming | hipEventDisableSystemFence;

// The engine's scratch (plan counts, pre-pass products, the pinned plan result) is shared by consecutive calls and is
// ordered only by the stream they are issued on.  A caller that moves to ANOTHER stream is made to wait for everything
// the engine still has in flight on the previous one (and on the side stream, which joins it): every call records, when
// it has enqueued its last work, an event on ITS OWN stream (StreamScope), and a call that finds itself on another
// stream than the last waits for that event.  The previous stream's handle is only ever compared, never used: the caller
// may have destroyed that stream since (the header allows it), and a handle that has been recycled for a new stream would
// otherwise have an event recorded on it that orders nothing.
pg_status enter_stream(pg_engine *e, hipStream_t st) {
    PG_HIP_TRY(hipSetDevice(e->device));
    if (e->have_last && e->last_stream != st) PG_HIP_TRY(hipStreamWaitEvent(st, e->ev_switch.get(), 0));
    e->last_stream = st;
    e->have_last = true;
    return PG_OK;
}
struct StreamScope {  // declared right after enter_stream succeeds; its destructor runs on every way out of the call
    pg_engine *e;
    hipStream_t st;
    ~StreamScope() { (void)hipEventRecord(e->ev_switch.get(), st); }
};

// Once a call has forked its pre-pass to the engine's side stream, the caller's stream waits for the side stream on EVERY way
// out of the call, the failing ones included: StreamScope (declared before, so destroyed after) then records ev_switch behind
// that wait, and a following call on another stream is ordered after the pre-pass, which writes e->d_prefix and variable slots.
struct SideJoin {
    pg_engine *e;
    hipStream_t st;
    bool forked = false, joined = false;
    ~SideJoin() {
        if (!forked || joined) return;
        (void)hipEventRecord(e->ev_inv.get(), e->side.get());
        (void)hipStreamWaitEvent(st, e->ev_inv.get(), 0);
    }
};

#ifndef PG_MIX_EARLY_TILES  // row tiles (256 items) per workgroup of the fused mix's arithmetic launch written during its inversions
#define PG_MIX_EARLY_TILES 1
#endif
#ifndef PG_INV_LANES_PER_CU  // lanes of the pre-pass per CU (256 = one wave per SIMD)
#define PG_INV_LANES_PER_CU 256
#endif
#ifndef PG_INV_MAX_PER_LANE
#define PG_INV_MAX_PER_LANE 32
#endif

// One batched gadget call = the emit kernel on the caller's stream and, for gadgets that invert, the inversion pre-pass
// on the engine's high-priority side stream.  The two write disjoint bytes (the pre-pass owns the inverse slots of
// the variable table), so they run concurrently; the caller's stream is made to wait for both before the call's
// results can be consumed.
// A split gadget (small items: the fused mix) = ONE launch that inverts and writes the variable table
// (scalar_mix_vars_kernel: integer arithmetic, bound by the multiplier) and then the rows, a pure store stream of 1.9 GB per
// 2^20 items.  The rows need nothing the arithmetic computes, and still the launches run ONE AFTER THE OTHER: side by
// side on the same compute units each slows the other down by more than the overlap gains, in every order and priority
// tried -- even with the arithmetic launch stripped of all its memory traffic -- and on disjoint compute units (CU-masked
// streams) the rows lack store bandwidth, which is per CU (profiles/NOTES_r03.md has the measurements).
// `planned`: the arithmetic launch makes the call's prefix sums itself (d_row_off / d_var_off are outputs, as are the
// engine's plan totals); otherwise it reads them.
pg_status launch_mix(pg_engine *e, const pg::ScalarMixArgs &A, const pg_columns *c, uint64_t batch, uint64_t gate_base,
                     uint64_t var_base, uint64_t zero_var, const uint64_t *row_off, const uint64_t *var_off, hipStream_t st,
                     const pg::MixPlan *planned, bool values_only = false) {
    using GD = pg::ScalarMixGD;
    PG_TRY(ensure_inv_scratch(e, batch));
    // geometry of the arithmetic launch: a wave owns 32 * ipl consecutive items; two waves per SIMD is what it is built for
    const uint64_t waves_wanted = (uint64_t)e->num_cus * 4 * 2;
    uint64_t ipl = (batch + waves_wanted * 32 - 1) / (waves_wanted * 32);
    if (ipl < 1) ipl = 1;
    if (ipl > pg::kMixMaxIpl) ipl = pg::kMixMaxIpl;
    const uint64_t waves = (batch + 32 * ipl - 1) / (32 * ipl);
    pg::EmitOut V = make_out(c, batch, GD::W, gate_base, var_base, zero_var, row_off, var_off);
    pg::EmitOut R = make_out(c, batch, GD::kRowsW, gate_base, var_base, zero_var, row_off, var_off);
    // early rows: the arithmetic launch's waiting waves write the first PG_MIX_EARLY_TILES row tiles of every workgroup's items
    // during its inversions (scalar_gadgets.hpp); the rows launches leave them alone.  Only where a workgroup holds enough tiles
    // for that to be a fraction of its rows (a small call's inversions are not worth hiding)
    const uint64_t span = (uint64_t)pg::kMixWaves * 32 * ipl;
    if (!values_only && ipl >= 8 && span <= 0xffffffffull) {
        V.early_span = R.early_span = (uint32_t)span;
        V.early_tiles = R.early_tiles = PG_MIX_EARLY_TILES;
    }
    const uint32_t max_blocks = (uint32_t)e->num_cus * PG_GRID_BLOCKS_PER_CU;
    const dim3 grid(R.tiles < max_blocks ? R.tiles : max_blocks), vgrid((uint32_t)((waves + pg::kMixWaves - 1) / pg::kMixWaves));
    const dim3 vblock(pg::kMixWaves * 64);
    uint4 *const prefix = e->d_prefix.as<uint4>(), *sink = prefix + e->inv_elems * 4 + 4 * 32 * 32 * 8;
    if (planned) {
        pg::MixPlan P = *planned;
        P.nwaves = vgrid.x;  // (the look-back is over workgroups)
        hipLaunchKernelGGL(pg::scalar_mix_vars_kernel<true>, vgrid, vblock, 0, st, A, V, (uint32_t)ipl, prefix, sink, P);
    } else
        hipLaunchKernelGGL(pg::scalar_mix_vars_kernel<false>, vgrid, vblock, 0, st, A, V, (uint32_t)ipl, prefix, sink,
                           pg::MixPlan{});
    if (values_only) {  // a witness refresh: the variable table (and, planned, the prefix sums) alone
        PG_HIP_TRY(hipGetLastError());
        return PG_OK;
    }
    hipLaunchKernelGGL(pg::rows_periodic_kernel<GD>, grid, dim3(pg::kThreads), 0, st, A, R);
    // the tiles that hold an item of another shape (none, unless an item stopped at its error): every other workgroup of
    // this launch reads two offsets and leaves
    hipLaunchKernelGGL((pg::emit_kernel<GD, pg::EMIT_ROWS>), grid, dim3(pg::kThreads), 0, st, A, R);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

// the witness refresh (EMIT_VALUES: the variable assignments alone) exists for every gadget of the one-launch emitter; the split
// gadget (the fused mix) has its own: the launch that writes its variable table, alone (launch_mix)
template <class GD> struct ValuesMode { static constexpr bool ok = !pg::Split<GD>::ok; };

template <class GD>
pg_status launch(pg_engine *e, const typename GD::Args &A, const pg_columns *c, uint64_t batch, uint64_t gate_base,
                 uint64_t var_base, uint64_t zero_var, const uint64_t *row_off, const uint64_t *var_off, void *stream,
                 const pg::MixPlan *planned = nullptr, bool values_only = false, uint32_t stride_rows = 0) {
    if ((batch + GD::W - 1) / GD::W > 0xffffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "batch too large for one call");
    if (stride_rows && (batch > 0xffffffffull || pg::Split<GD>::ok || GD::kRagged))
        return fail(PG_ERR_INVALID_ARGUMENT, "a row stride is for uniform one-launch gadgets of at most 2^32 - 1 items");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    if constexpr (pg::Split<GD>::ok) {
        return launch_mix(e, A, c, batch, gate_base, var_base, zero_var, row_off, var_off, st, planned, values_only);
    } else {
        pg::EmitOut O = make_out(c, batch, GD::W, gate_base, var_base, zero_var, row_off, var_off);
        if (stride_rows) {  // rows of other calls between the items: one item per tile (emit.hpp)
            O.stride_rows = stride_rows;
            O.tiles = (uint32_t)batch;
        }
        bool side = false;  // the inversion pre-pass runs on the engine's side stream
        SideJoin join{e, st};
        if constexpr (GD::kInv > 0) {
            constexpr int GRP = GD::kInvGroup;
            const uint64_t elems = batch * GD::kInv;
            PG_TRY(ensure_inv_scratch(e, elems));
            const uint64_t lanes_wanted = (uint64_t)e->num_cus * PG_INV_LANES_PER_CU;
            uint64_t per_lane = (elems + lanes_wanted - 1) / lanes_wanted;
            if (per_lane < 1) per_lane = 1;
            if (per_lane > PG_INV_MAX_PER_LANE) per_lane = PG_INV_MAX_PER_LANE;
            const uint64_t groups = (per_lane + GRP - 1) / GRP;  // a lane owns groups * GRP elements
            const uint64_t lanes = (elems + groups * GRP - 1) / (groups * GRP);
            const uint32_t blocks = (uint32_t)((lanes + pg::kThreads - 1) / pg::kThreads);
            // a handful of elements (the single-gadget calls of pg_composer): two event hops cost more than the overlap buys.
            // A big call (an emit launch of milliseconds): the pre-pass goes FIRST on the caller's stream -- beside the
            // emitter its round trips crawl through a saturated memory system and it ends with the emitter (17.58 of 17.64 ms
            // at 2^20 ragged max_bound items), one wave per SIMD taken from the store stream all the while; alone it takes
            // 0.15 ms and the step is the same within 0.4 % (profiles/NOTES_r04.md, tools/c4_timeline.sh).
            side = elems >= 2048 && elems < (1ull << 18);
            hipStream_t inv_st = st;
            if (side) {
                PG_HIP_TRY(hipEventRecord(e->ev_fork.get(), st));  // the pre-pass reads the call's inputs: order it after the stream
                PG_HIP_TRY(hipStreamWaitEvent(e->side.get(), e->ev_fork.get(), 0));
                join.forked = true;
                inv_st = e->side.get();
            }
            if constexpr (pg::InvDense<GD>::ok) {
                O.inv_dense = e->d_prefix.as<uint4>();
                O.inv_elems = elems;
                O.inv_in_place = side;  // else the pre-pass is through before the emitter starts: it leaves the inverses where it computed them
            }
            hipLaunchKernelGGL((pg::batch_invert_kernel<GD, GRP>), dim3(blocks), dim3(pg::kThreads), 0, inv_st, A, O, elems,
                               (uint32_t)groups, e->d_prefix.as<uint4>());
            PG_HIP_TRY(hipGetLastError());
            if (side) PG_HIP_TRY(hipEventRecord(e->ev_inv.get(), e->side.get()));
        }
        const uint32_t max_blocks = (uint32_t)e->num_cus * (values_only ? PG_GRID_BLOCKS_PER_CU : PG_EMIT_GRID_BLOCKS_PER_CU);
        const dim3 egrid(O.tiles < max_blocks ? O.tiles : max_blocks);
        if (values_only) {
            if constexpr (ValuesMode<GD>::ok) hipLaunchKernelGGL((pg::emit_kernel<GD, pg::EMIT_VALUES>), egrid, dim3(pg::kThreads), 0, st, A, O);
            else return fail(PG_ERR_INVALID_ARGUMENT, "this gadget has no values-only emission");
        } else {
            hipLaunchKernelGGL(pg::emit_kernel<GD>, egrid, dim3(pg::kThreads), 0, st, A, O);
        }
        PG_HIP_TRY(hipGetLastError());
        if (side) {
            PG_HIP_TRY(hipStreamWaitEvent(st, e->ev_inv.get(), 0));  // join
            join.joined = true;
        }
        return PG_OK;
    }
}

// a uniform gadget without inverses in the emitter mode the caller names: one launch on the caller's stream
template <class GD, int MODE>
pg_status launch_mode(pg_engine *e, const typename GD::Args &A, const pg_columns *c, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                      uint64_t zero_var, void *stream) {
    static_assert(GD::kInv == 0 && !GD::kRagged && !pg::Split<GD>::ok, "one launch, no pre-pass, no prefix sums");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    const pg::EmitOut O = make_out(c, batch, GD::W, gate_base, var_base, zero_var, nullptr, nullptr);
    const uint32_t max_blocks = (uint32_t)e->num_cus * (MODE == pg::EMIT_VALUES ? PG_GRID_BLOCKS_PER_CU : PG_EMIT_GRID_BLOCKS_PER_CU);
    hipLaunchKernelGGL((pg::emit_kernel<GD, MODE>), dim3(O.tiles < max_blocks ? O.tiles : max_blocks), dim3(pg::kThreads), 0, st, A, O);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status scalar_args(const pg_variable *a_var, const pg_scalar *a_val, const pg_variable *b_var,
                             const pg_scalar *b_val, pg_variable *res, pg::ScalarArgs *A) {
    PG_TRY(check_u64s(a_var, "first Variable array"));
    PG_TRY(check_u64s(b_var, "second Variable array"));
    PG_TRY(check_scalars(a_val, "first value array"));
    PG_TRY(check_scalars(b_val, "second value array"));
    PG_TRY(check_u64s(res, "d_result_vars", true));
    A->a_var = a_var;
    A->b_var = b_var;
    A->a_val = reinterpret_cast<const uint4 *>(a_val);
    A->b_val = reinterpret_cast<const uint4 *>(b_val);
    A->result_vars = res;
    A->err_mask = nullptr;
    return PG_OK;
}

// the launches of an asynchronous plan of a gadget with failing items (scratch ensured, arguments checked by the caller)
template <class PlanKernel>
pg_status error_plan_launch(pg_engine *e, PlanKernel kernel, const pg_scalar *d_value, uint64_t batch, uint64_t *d_row_off,
                            uint64_t *d_var_off, uint8_t *d_err_mask, hipStream_t st) {
    const uint32_t grid = (uint32_t)((batch + pg::kScanBlock - 1) / pg::kScanBlock);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(pg::kThreads), 0, st, reinterpret_cast<const uint4 *>(d_value), batch,
                       e->d_rows.as<uint32_t>(), e->d_vars.as<uint32_t>(), d_err_mask, e->d_err_count.as<uint32_t>(),
                       plan_scan(e, batch, d_row_off, d_var_off, true));
    PG_HIP_TRY(hipGetLastError());
    return scan_counts(e, batch, d_row_off, d_var_off, nullptr, nullptr, st, true);
}

// out == NULL: asynchronous form (results through pg_plan_result)
template <class PlanKernel>
pg_status error_plan(pg_engine *e, PlanKernel kernel, const pg_scalar *d_value, uint64_t batch, uint64_t *d_row_off,
                            uint64_t *d_var_off, uint8_t *d_err_mask, pg_layout *out, uint64_t *err_count, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (out) std::memset(out, 0, sizeof *out);
    if (err_count) *err_count = 0;
    if (batch == 0) {  // stream-ordered like every other write of the plan result
        PG_TRY(enter_stream(e, static_cast<hipStream_t>(stream)));
        StreamScope scope{e, static_cast<hipStream_t>(stream)};
        PG_HIP_TRY(hipMemsetAsync(e->plan(), 0, sizeof(pg_engine::PlanResult), static_cast<hipStream_t>(stream)));
        return PG_OK;
    }
    PG_TRY(check_scalars(d_value, "value array"));
    PG_TRY(check_u64s(d_row_off, "d_row_off"));
    PG_TRY(check_u64s(d_var_off, "d_var_off"));
    PG_TRY(ensure_scratch(e, batch));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    if (!out) return error_plan_launch(e, kernel, d_value, batch, d_row_off, d_var_off, d_err_mask, st);
    // e->d_err_count is zero between calls: whoever reads it (scan_final_kernel, the bulk decoder) leaves it so
    const uint32_t grid = (uint32_t)((batch + pg::kScanBlock - 1) / pg::kScanBlock);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(pg::kThreads), 0, st, reinterpret_cast<const uint4 *>(d_value), batch,
                       e->d_rows.as<uint32_t>(), e->d_vars.as<uint32_t>(), d_err_mask, e->d_err_count.as<uint32_t>(),
                       plan_scan(e, batch, d_row_off, d_var_off, true));
    PG_HIP_TRY(hipGetLastError());
    PG_TRY(scan_counts(e, batch, d_row_off, d_var_off, &out->n_gates, &out->n_vars, st, true));
    const uint32_t errs = e->plan()->errs;
    if (err_count) *err_count = errs;
    if (errs) return fail(PG_ERR_NON_EXISTING_INVERSE, std::to_string(errs) + " item(s) have no inverse (value = 0)");
    return PG_OK;
}

}  // namespace

extern "C" {

const char *pg_status_string(pg_status s) {
    switch (s) {
        case PG_OK: return "ok";
        case PG_ERR_NON_EXISTING_INVERSE: return "non-existing inverse";
        case PG_ERR_INVALID_ARGUMENT: return "invalid argument";
        case PG_ERR_NO_DEVICE: return "no usable gfx950 device";
        case PG_ERR_HIP: return "HIP runtime error";
        case PG_ERR_CAPACITY: return "composer capacity exceeded";
        case PG_ERR_BAD_ENCODING: return "encoding not below the modulus";
    }
    return "unknown status";
}

const char *pg_last_error(void) { return g_last_error.c_str(); }
const char *pg_build_arch(void) { return "gfx950"; }

pg_status pg_engine_create(int device, pg_engine **out) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PG_ERR_NO_DEVICE, "hipGetDeviceCount found no device: this library has no CPU path");
    if (device < 0 || device >= count) return fail(PG_ERR_INVALID_ARGUMENT, "device index out of range");
    hipDeviceProp_t prop;
    PG_HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PG_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", library is built for gfx950 only");
    PG_HIP_TRY(hipSetDevice(device));
    std::unique_ptr<pg_engine> e(new (std::nothrow) pg_engine());
    if (!e) return fail(PG_ERR_HIP, "out of host memory");
    e->device = device;
    e->num_cus = prop.multiProcessorCount;
    if (e->d_pow2.reserve(256 * 2 * sizeof(uint4)) != PG_OK) return fail(PG_ERR_HIP, "hipMalloc(pow2 table) failed");
    if (e->h_plan.reserve(2 * sizeof(pg_engine::PlanResult)) != PG_OK) return fail(PG_ERR_HIP, "hipHostMalloc(plan result) failed");
    *e->plan() = pg_engine::PlanResult{0, 0, 0, 0};
    *e->bad_encodings() = 0;
    // the pre-pass is the critical path of a call with small items: highest priority, so its waves are placed ahead of
    // the rows-only emit launch it runs beside
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
#if defined(PG_SIDE_STREAM_NORMAL_PRIORITY)
    prio_hi = 0;
#endif
    if (e->side.create_with_priority(hipStreamNonBlocking, prio_hi) != PG_OK || e->ev_fork.create(kOrderingEvent) != PG_OK ||
        e->ev_inv.create(kOrderingEvent) != PG_OK || e->ev_switch.create(kOrderingEvent) != PG_OK)
        return fail(PG_ERR_HIP, "creating the engine's side stream / events failed");
    hipLaunchKernelGGL(pg::pow2_table_kernel, dim3(1), dim3(64), 0, nullptr, e->d_pow2.as<uint4>());
    hipError_t err = hipDeviceSynchronize();
    if (err != hipSuccess) return fail(PG_ERR_HIP, std::string("pow2 table kernel: ") + hipGetErrorString(err));
    *out = e.release();
    return PG_OK;
}

// ordering only: the engine's device current, the side stream and the last copy out of `seg` drained.  The members release themselves.
void pg_engine_destroy(pg_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->side.get());
    (void)e->seg.wait();
    delete e;
}

pg_status pg_engine_sync(pg_engine *e, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    PG_HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return PG_OK;
}

/* ---- encodings, in bulk ---------------------------------------------------- */
pg_status pg_scalars_from_canonical_batch(pg_engine *e, const void *d_bytes, uint64_t batch, pg_scalar *d_out, uint8_t *d_bad_mask,
                                          uint64_t *bad_count, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (bad_count) *bad_count = 0;
    if (batch == 0) return PG_OK;
    PG_TRY(check_scalars(d_bytes, "d_bytes"));
    PG_TRY(check_scalars(d_out, "d_out"));
    PG_TRY(ensure_scratch(e, 1));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // e->d_err_count is the plan kernels' too: behind a plan still pending on another stream
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    uint32_t *const d_errs = e->d_err_count.as<uint32_t>();
    PG_HIP_TRY(hipMemsetAsync(d_errs, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(pg::from_canonical_kernel, dim3((uint32_t)((batch + pg::kThreads - 1) / pg::kThreads)), dim3(pg::kThreads), 0, st,
                       static_cast<const uint4 *>(d_bytes), batch, reinterpret_cast<uint4 *>(d_out), d_bad_mask, d_errs);
    PG_HIP_TRY(hipGetLastError());
    PG_HIP_TRY(hipMemcpyAsync(e->bad_encodings(), d_errs, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PG_HIP_TRY(hipMemsetAsync(d_errs, 0, sizeof(uint32_t), st));  // zero between calls (see error_plan)
    PG_HIP_TRY(hipStreamSynchronize(st));
    const uint32_t bad = *e->bad_encodings();
    if (bad_count) *bad_count = bad;
    if (bad) return fail(PG_ERR_BAD_ENCODING, std::to_string(bad) + " encoding(s) are not below the modulus");
    return PG_OK;
}

pg_status pg_scalars_to_canonical_batch(pg_engine *e, const pg_scalar *d_scalars, uint64_t batch, void *d_bytes, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    PG_TRY(check_scalars(d_scalars, "d_scalars"));
    PG_TRY(check_scalars(d_bytes, "d_bytes"));
    PG_HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(pg::to_canonical_kernel, dim3((uint32_t)((batch + pg::kThreads - 1) / pg::kThreads)), dim3(pg::kThreads), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const uint4 *>(d_scalars), batch, static_cast<uint4 *>(d_bytes));
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

/* ---- host scalar helpers ------------------------------------------------ */
void pg_scalar_from_u64(uint64_t v, pg_scalar *out) { from_fr(pg::fr_from_u64(v), out); }
void pg_scalar_from_canonical(const uint64_t raw[4], pg_scalar *out) {
    from_fr(pg::fr_to_mont(pg::Fr{{raw[0], raw[1], raw[2], raw[3]}}), out);
}
void pg_scalar_to_canonical(const pg_scalar *s, uint64_t raw[4]) {
    pg::Fr c = pg::fr_from_mont(to_fr(s));
    std::memcpy(raw, c.l, sizeof c.l);
}
void pg_scalar_add(const pg_scalar *a, const pg_scalar *b, pg_scalar *out) { from_fr(pg::fr_add(to_fr(a), to_fr(b)), out); }
void pg_scalar_sub(const pg_scalar *a, const pg_scalar *b, pg_scalar *out) { from_fr(pg::fr_sub(to_fr(a), to_fr(b)), out); }
void pg_scalar_neg(const pg_scalar *a, pg_scalar *out) { from_fr(pg::fr_neg(to_fr(a)), out); }
void pg_scalar_mul(const pg_scalar *a, const pg_scalar *b, pg_scalar *out) { from_fr(pg::fr_mul(to_fr(a), to_fr(b)), out); }
pg_status pg_scalar_invert(const pg_scalar *a, pg_scalar *out) {
    if (!a || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_reduced(to_fr(a))) return fail(PG_ERR_INVALID_ARGUMENT, "scalar is not a reduced BlsScalar");
    from_fr(pg::fr_invert_or_zero(to_fr(a)), out);
    return pg::fr_is_zero(to_fr(a)) ? fail(PG_ERR_NON_EXISTING_INVERSE, "zero has no inverse") : PG_OK;
}
pg_status pg_scalar_invert_fermat(const pg_scalar *a, pg_scalar *out) {
    if (!a || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!is_reduced(to_fr(a))) return fail(PG_ERR_INVALID_ARGUMENT, "scalar is not a reduced BlsScalar");
    from_fr(pg::fr_invert_fermat(to_fr(a)), out);
    return pg::fr_is_zero(to_fr(a)) ? fail(PG_ERR_NON_EXISTING_INVERSE, "zero has no inverse") : PG_OK;
}
uint64_t pg_bits_count(const pg_scalar *s) { return pg::bits_count(to_fr(s)); }
uint64_t pg_num_bits_closest_power_of_two(const pg_scalar *s) { return pg::num_bits_closest_power_of_two(to_fr(s)); }

/* ---- range_check ---------------------------------------------------------- */
pg_status pg_range_check_layout(const pg_scalar *min_range, const pg_scalar *max_range, uint64_t batch, pg_layout *out) {
    if (!min_range || !max_range || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    pg::Fr mn = to_fr(min_range), mx = to_fr(max_range);
    if (!is_reduced(mn) || !is_reduced(mx)) return fail(PG_ERR_INVALID_ARGUMENT, "bound is not a reduced BlsScalar");
    // range.rs:87-90
    uint64_t n = pg::num_bits_closest_power_of_two(pg::fr_sub(mx, pg::fr_one()));
    out->num_bits = n;
    out->gates_per_item = pg::kind_rows(pg::WIRES_RANGE_CHECK, n);
    out->vars_per_item = pg::kind_vars(pg::WIRES_RANGE_CHECK, n);  // those of range_check and the one of allocate
    out->n_gates = out->gates_per_item * batch;
    out->n_vars = out->vars_per_item * batch;
    return PG_OK;
}

static pg_status range_check_common(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range,
                                    const pg_variable *d_witness_var, const pg_scalar *d_witness, uint64_t batch,
                                    uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                    pg_variable *d_result_vars, void *stream, bool values_only = false, uint32_t stride_rows = 0) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    pg_layout lay;
    PG_TRY(pg_range_check_layout(min_range, max_range, batch, &lay));
    if (batch == 0) return PG_OK;
    PG_TRY(check_scalars(d_witness, "d_witness"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    PG_TRY(check_columns(out));
    if (lay.num_bits < 2 || lay.num_bits > 255) return fail(PG_ERR_INVALID_ARGUMENT, "ladder length out of range");
    pg::RangeCheckGD::Args A{};
    A.min_range = to_fr(min_range);
    A.max_range = to_fr(max_range);
    A.n = (uint32_t)lay.num_bits;
    A.witness = reinterpret_cast<const uint4 *>(d_witness);
    A.witness_vars = d_witness_var;
    A.result_vars = d_result_vars;
    A.pow2 = e->d_pow2.as<uint4>();
    return launch<pg::RangeCheckGD>(e, A, out, batch, gate_base, var_base, 0, nullptr, nullptr, stream, nullptr, values_only, stride_rows);
}

// a witness refresh's `out`: only var_values is written (EMIT_VALUES); the row pointers merely have to pass the checks
static pg_columns values_columns(pg_scalar *d_var_values) {
    pg_columns c;
    c.q_m = c.q_l = c.q_r = c.q_o = c.q_c = c.var_values = d_var_values;
    c.w_l = c.w_r = c.w_o = reinterpret_cast<uint64_t *>(d_var_values);
    return c;
}

pg_status pg_range_check_values_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range, const pg_scalar *d_witness,
                                      uint64_t batch, pg_scalar *d_var_values, void *stream) {
    const pg_columns c = values_columns(d_var_values);
    return range_check_common(e, min_range, max_range, nullptr, d_witness, batch, 0, 0, &c, nullptr, stream, true);
}

pg_status pg_range_check_structure_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range, uint64_t batch,
                                         uint64_t gate_base, uint64_t var_base, const pg_columns *out, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    pg_layout lay;
    PG_TRY(pg_range_check_layout(min_range, max_range, batch, &lay));
    if (batch == 0) return PG_OK;
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "columns are NULL");
    pg_columns c = *out;
    if (!c.var_values) c.var_values = c.q_m;  // never written: only has to pass the pointer checks
    PG_TRY(check_columns(&c));
    if (lay.num_bits < 2 || lay.num_bits > 255) return fail(PG_ERR_INVALID_ARGUMENT, "ladder length out of range");
    if ((batch + pg::RangeCheckGD::W - 1) / pg::RangeCheckGD::W > 0xffffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "batch too large for one call");
    PG_HIP_TRY(hipSetDevice(e->device));
    pg::RangeCheckGD::Args A{};
    A.min_range = to_fr(min_range);
    A.max_range = to_fr(max_range);
    A.n = (uint32_t)lay.num_bits;
    A.pow2 = e->d_pow2.as<uint4>();
    const pg::EmitOut O = make_out(&c, batch, pg::RangeCheckGD::W, gate_base, var_base, 0, nullptr, nullptr);
    const uint32_t max_blocks = (uint32_t)e->num_cus * PG_GRID_BLOCKS_PER_CU;
    hipLaunchKernelGGL((pg::emit_kernel<pg::RangeCheckGD, pg::EMIT_STRUCTURE>), dim3(grid_cap(O.tiles, max_blocks)), dim3(pg::kThreads), 0,
                       static_cast<hipStream_t>(stream), A, O);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_range_check_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range,
                               const pg_scalar *d_witness, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                               const pg_columns *out, pg_variable *d_result_vars, void *stream) {
    return range_check_common(e, min_range, max_range, nullptr, d_witness, batch, gate_base, var_base, out, d_result_vars, stream);
}

pg_status pg_range_check_allocated_batch(pg_engine *e, const pg_scalar *min_range, const pg_scalar *max_range,
                                         const pg_variable *d_witness_var, const pg_scalar *d_witness, uint64_t batch,
                                         uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                         pg_variable *d_result_vars, void *stream) {
    if (batch) PG_TRY(check_u64s(d_witness_var, "d_witness_var"));
    return range_check_common(e, min_range, max_range, d_witness_var, d_witness, batch, gate_base, var_base, out,
                              d_result_vars, stream);
}

/* ---- scalar_decomposition_gadget -------------------------------------------- */
pg_status pg_scalar_decomposition_layout(uint64_t num_bits, uint64_t batch, pg_layout *out) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (num_bits > 256) return fail(PG_ERR_INVALID_ARGUMENT, "num_bits > 256 (the reference panics: src/range.rs:134)");
    out->num_bits = num_bits;
    out->gates_per_item = pg::kind_rows(pg::WIRES_DECOMPOSITION, num_bits);
    out->vars_per_item = pg::kind_vars(pg::WIRES_DECOMPOSITION, num_bits);
    out->n_gates = out->gates_per_item * batch;
    out->n_vars = out->vars_per_item * batch;
    return PG_OK;
}

static pg_status decomposition_common(pg_engine *e, uint64_t num_bits, const pg_variable *d_witness_var,
                                      const pg_scalar *d_witness, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                      const pg_columns *out, pg_variable *d_result_vars, void *stream, bool values_only) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    pg_layout lay;
    PG_TRY(pg_scalar_decomposition_layout(num_bits, batch, &lay));
    if (batch == 0) return PG_OK;
    PG_TRY(check_u64s(d_witness_var, "d_witness_var"));
    PG_TRY(check_scalars(d_witness, "d_witness"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    PG_TRY(check_columns(out));
    pg::DecompositionGD::Args A{};
    A.n = (uint32_t)num_bits;
    A.witness = reinterpret_cast<const uint4 *>(d_witness);
    A.witness_vars = d_witness_var;
    A.result_vars = d_result_vars;
    A.pow2 = e->d_pow2.as<uint4>();
    return launch<pg::DecompositionGD>(e, A, out, batch, gate_base, var_base, 0, nullptr, nullptr, stream, nullptr, values_only);
}

pg_status pg_scalar_decomposition_batch(pg_engine *e, uint64_t num_bits, const pg_variable *d_witness_var,
                                        const pg_scalar *d_witness, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                        const pg_columns *out, pg_variable *d_result_vars, void *stream) {
    return decomposition_common(e, num_bits, d_witness_var, d_witness, batch, gate_base, var_base, out, d_result_vars, stream, false);
}

/* ---- max_bound ------------------------------------------------------------ */
pg_status pg_max_bound_layout(const pg_scalar *max_range, uint64_t batch, pg_layout *out) {
    if (!max_range || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    pg::Fr mx = to_fr(max_range);
    if (!is_reduced(mx)) return fail(PG_ERR_INVALID_ARGUMENT, "bound is not a reduced BlsScalar");
    uint64_t n = pg::num_bits_closest_power_of_two(pg::fr_sub(mx, pg::fr_one()));
    out->num_bits = n;
    out->gates_per_item = pg::kind_rows(pg::WIRES_MAX_BOUND, n);
    out->vars_per_item = pg::kind_vars(pg::WIRES_MAX_BOUND, n);  // those of max_bound and the one of allocate
    out->n_gates = out->gates_per_item * batch;
    out->n_vars = out->vars_per_item * batch;
    return PG_OK;
}

static pg_status max_bound_common(pg_engine *e, const pg_scalar *max_range, const pg_variable *d_witness_var,
                                  const pg_scalar *d_witness, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                  const pg_columns *out, pg_variable *d_result_vars, void *stream, bool values_only = false,
                                  uint32_t stride_rows = 0) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    pg_layout lay;
    PG_TRY(pg_max_bound_layout(max_range, batch, &lay));
    if (batch == 0) return PG_OK;
    PG_TRY(check_scalars(d_witness, "d_witness"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    PG_TRY(check_columns(out));
    pg::MaxBoundGD<false>::Args A{};
    A.max_range = to_fr(max_range);
    A.n = (uint32_t)lay.num_bits;
    A.witness = reinterpret_cast<const uint4 *>(d_witness);
    A.witness_vars = d_witness_var;
    A.result_vars = d_result_vars;
    A.pow2 = e->d_pow2.as<uint4>();
    return launch<pg::MaxBoundGD<false>>(e, A, out, batch, gate_base, var_base, 0, nullptr, nullptr, stream, nullptr, values_only, stride_rows);
}

pg_status pg_max_bound_values_batch(pg_engine *e, const pg_scalar *max_range, const pg_scalar *d_witness, uint64_t batch,
                                    pg_scalar *d_var_values, void *stream) {
    const pg_columns c = values_columns(d_var_values);
    return max_bound_common(e, max_range, nullptr, d_witness, batch, 0, 0, &c, nullptr, stream, true);
}

pg_status pg_max_bound_batch(pg_engine *e, const pg_scalar *max_range, const pg_scalar *d_witness, uint64_t batch,
                             uint64_t gate_base, uint64_t var_base, const pg_columns *out, pg_variable *d_result_vars,
                             void *stream) {
    return max_bound_common(e, max_range, nullptr, d_witness, batch, gate_base, var_base, out, d_result_vars, stream);
}

pg_status pg_max_bound_allocated_batch(pg_engine *e, const pg_scalar *max_range, const pg_variable *d_witness_var,
                                       const pg_scalar *d_witness, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                       const pg_columns *out, pg_variable *d_result_vars, void *stream) {
    if (batch) PG_TRY(check_u64s(d_witness_var, "d_witness_var"));
    return max_bound_common(e, max_range, d_witness_var, d_witness, batch, gate_base, var_base, out, d_result_vars, stream);
}

}  // extern "C"

// the plan of a batch with one upper bound per item; KIND: what an item weighs (max_bound, or range_check: two blocks on max's ladder length)
template <uint32_t KIND>
static pg_status bound_ragged_plan_common(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                          uint64_t *d_row_off, uint64_t *d_var_off, pg_layout *out, void *stream) {
    // (a fused plan's published prefixes hold 31 bits of rows and of variables, emit.hpp: blocks x 1024 items x the largest item --
    // 2048 blocks for max_bound's 517, 2028 for range_check's 1034)
    constexpr uint64_t kLargest = std::max(pg::kind_rows(KIND, 255), pg::kind_vars(KIND, 255));
    constexpr uint32_t kFused = (uint32_t)std::min<uint64_t>(pg::kPlanFusedBlocks, ((1ull << 31) - 1) / (pg::kScanBlock * kLargest));
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (out) std::memset(out, 0, sizeof *out);
    if (batch == 0) {
        PG_TRY(enter_stream(e, static_cast<hipStream_t>(stream)));
        StreamScope scope{e, static_cast<hipStream_t>(stream)};
        PG_HIP_TRY(hipMemsetAsync(e->plan(), 0, sizeof(pg_engine::PlanResult), static_cast<hipStream_t>(stream)));
        return PG_OK;
    }
    PG_TRY(check_scalars(d_max_range, "d_max_range"));
    if (!d_num_bits || !aligned(d_num_bits, 4)) return fail(PG_ERR_INVALID_ARGUMENT, "d_num_bits NULL or misaligned");
    PG_TRY(check_u64s(d_row_off, "d_row_off"));
    PG_TRY(check_u64s(d_var_off, "d_var_off"));
    PG_TRY(ensure_scratch(e, batch));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    const uint32_t grid = (uint32_t)((batch + pg::kScanBlock - 1) / pg::kScanBlock);
    hipLaunchKernelGGL(pg::max_bound_plan_kernel<KIND>, dim3(grid), dim3(pg::kThreads), 0, st,
                       reinterpret_cast<const uint4 *>(d_max_range), batch, e->d_pow2.as<uint4>(), d_num_bits, e->d_rows.as<uint32_t>(),
                       e->d_vars.as<uint32_t>(), plan_scan(e, batch, d_row_off, d_var_off, false, kFused));
    PG_HIP_TRY(hipGetLastError());
    // a max_bound plan has no failing items: the scan writes errs = 0 with the totals, in stream order
    if (!out) return scan_counts(e, batch, d_row_off, d_var_off, nullptr, nullptr, st, false, kFused);
    PG_TRY(scan_counts(e, batch, d_row_off, d_var_off, &out->n_gates, &out->n_vars, st, false, kFused));
    return PG_OK;
}
static pg_status max_bound_ragged_plan_common(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                              uint64_t *d_row_off, uint64_t *d_var_off, pg_layout *out, void *stream) {
    return bound_ragged_plan_common<pg::WIRES_MAX_BOUND>(e, d_max_range, batch, d_num_bits, d_row_off, d_var_off, out, stream);
}

extern "C" {

pg_status pg_max_bound_ragged_plan(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                   uint64_t *d_row_off, uint64_t *d_var_off, pg_layout *out, void *stream) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return max_bound_ragged_plan_common(e, d_max_range, batch, d_num_bits, d_row_off, d_var_off, out, stream);
}

pg_status pg_max_bound_ragged_plan_async(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                         uint64_t *d_row_off, uint64_t *d_var_off, void *stream) {
    return max_bound_ragged_plan_common(e, d_max_range, batch, d_num_bits, d_row_off, d_var_off, nullptr, stream);
}

pg_status pg_plan_result(pg_engine *e, pg_layout *out, uint64_t *err_count) {
    if (!e || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    std::memset(out, 0, sizeof *out);
    PG_TRY(plan_totals(e, &out->n_gates, &out->n_vars));
    if (err_count) *err_count = e->plan()->errs;
    return e->plan()->errs ? fail(PG_ERR_NON_EXISTING_INVERSE, std::to_string(e->plan()->errs) + " item(s) have no inverse")
                           : PG_OK;
}

static pg_status max_bound_ragged_common(pg_engine *e, const pg_scalar *d_max_range, const pg_scalar *d_witness, uint64_t batch,
                                         const uint32_t *d_num_bits, const uint64_t *d_row_off, const uint64_t *d_var_off,
                                         uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                         pg_variable *d_result_vars, void *stream, bool values_only) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    PG_TRY(check_scalars(d_max_range, "d_max_range"));
    PG_TRY(check_scalars(d_witness, "d_witness"));
    if (!d_num_bits) return fail(PG_ERR_INVALID_ARGUMENT, "d_num_bits is NULL");
    PG_TRY(check_u64s(d_row_off, "d_row_off"));
    PG_TRY(check_u64s(d_var_off, "d_var_off"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    PG_TRY(check_columns(out));
    pg::MaxBoundGD<true>::Args A{};
    A.max_range_v = reinterpret_cast<const uint4 *>(d_max_range);
    A.num_bits_v = d_num_bits;
    A.witness = reinterpret_cast<const uint4 *>(d_witness);
    A.result_vars = d_result_vars;
    A.pow2 = e->d_pow2.as<uint4>();
    return launch<pg::MaxBoundGD<true>>(e, A, out, batch, gate_base, var_base, 0, d_row_off, d_var_off, stream, nullptr, values_only);
}

pg_status pg_max_bound_ragged_batch(pg_engine *e, const pg_scalar *d_max_range, const pg_scalar *d_witness, uint64_t batch,
                                    const uint32_t *d_num_bits, const uint64_t *d_row_off, const uint64_t *d_var_off,
                                    uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                    pg_variable *d_result_vars, void *stream) {
    return max_bound_ragged_common(e, d_max_range, d_witness, batch, d_num_bits, d_row_off, d_var_off, gate_base, var_base, out,
                                   d_result_vars, stream, false);
}

pg_status pg_max_bound_ragged_values_batch(pg_engine *e, const pg_scalar *d_max_range, const pg_scalar *d_witness, uint64_t batch,
                                           const uint32_t *d_num_bits, const uint64_t *d_row_off, const uint64_t *d_var_off,
                                           pg_scalar *d_var_values, void *stream) {
    const pg_columns c = values_columns(d_var_values);
    return max_bound_ragged_common(e, d_max_range, d_witness, batch, d_num_bits, d_row_off, d_var_off, 0, 0, &c, nullptr, stream, true);
}

/* ---- range_check, one (min, max) pair per item ------------------------------ */
pg_status pg_range_check_ragged_plan(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                     uint64_t *d_row_off, uint64_t *d_var_off, pg_layout *out, void *stream) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return bound_ragged_plan_common<pg::WIRES_RANGE_CHECK>(e, d_max_range, batch, d_num_bits, d_row_off, d_var_off, out, stream);
}

pg_status pg_range_check_ragged_plan_async(pg_engine *e, const pg_scalar *d_max_range, uint64_t batch, uint32_t *d_num_bits,
                                           uint64_t *d_row_off, uint64_t *d_var_off, void *stream) {
    return bound_ragged_plan_common<pg::WIRES_RANGE_CHECK>(e, d_max_range, batch, d_num_bits, d_row_off, d_var_off, nullptr, stream);
}

static pg_status range_check_ragged_common(pg_engine *e, const pg_scalar *d_min_range, const pg_scalar *d_max_range,
                                           const pg_scalar *d_witness, uint64_t batch, const uint32_t *d_num_bits,
                                           const uint64_t *d_row_off, const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base,
                                           const pg_columns *out, pg_variable *d_result_vars, void *stream, bool values_only) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    PG_TRY(check_scalars(d_min_range, "d_min_range"));
    PG_TRY(check_scalars(d_max_range, "d_max_range"));
    PG_TRY(check_scalars(d_witness, "d_witness"));
    if (!d_num_bits) return fail(PG_ERR_INVALID_ARGUMENT, "d_num_bits is NULL");
    PG_TRY(check_u64s(d_row_off, "d_row_off"));
    PG_TRY(check_u64s(d_var_off, "d_var_off"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    PG_TRY(check_columns(out));
    pg::RangeBoundsGD::Args A{};
    A.min_range_v = reinterpret_cast<const uint4 *>(d_min_range);
    A.max_range_v = reinterpret_cast<const uint4 *>(d_max_range);
    A.num_bits_v = d_num_bits;
    A.witness = reinterpret_cast<const uint4 *>(d_witness);
    A.result_vars = d_result_vars;
    A.pow2 = e->d_pow2.as<uint4>();
    return launch<pg::RangeBoundsGD>(e, A, out, batch, gate_base, var_base, 0, d_row_off, d_var_off, stream, nullptr, values_only);
}

pg_status pg_range_check_ragged_batch(pg_engine *e, const pg_scalar *d_min_range, const pg_scalar *d_max_range,
                                      const pg_scalar *d_witness, uint64_t batch, const uint32_t *d_num_bits,
                                      const uint64_t *d_row_off, const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base,
                                      const pg_columns *out, pg_variable *d_result_vars, void *stream) {
    return range_check_ragged_common(e, d_min_range, d_max_range, d_witness, batch, d_num_bits, d_row_off, d_var_off, gate_base, var_base,
                                     out, d_result_vars, stream, false);
}

pg_status pg_range_check_ragged_values_batch(pg_engine *e, const pg_scalar *d_min_range, const pg_scalar *d_max_range,
                                             const pg_scalar *d_witness, uint64_t batch, const uint32_t *d_num_bits,
                                             const uint64_t *d_row_off, const uint64_t *d_var_off, pg_scalar *d_var_values,
                                             void *stream) {
    const pg_columns c = values_columns(d_var_values);
    return range_check_ragged_common(e, d_min_range, d_max_range, d_witness, batch, d_num_bits, d_row_off, d_var_off, 0, 0, &c, nullptr,
                                     stream, true);
}

/* ---- scalar gadgets ------------------------------------------------------- */
}  // extern "C"

// the three gadgets on two existing Variables each; values_only: a witness refresh (pg_composer_clear_witness)
template <class GD>
static pg_status two_input_common(pg_engine *e, const pg_variable *d_a_var, const pg_scalar *d_a_val, const pg_variable *d_b_var,
                                  const pg_scalar *d_b_val, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                                  const pg_columns *out, pg_variable *d_result_vars, void *stream, bool values_only) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    pg::ScalarArgs A;
    PG_TRY(scalar_args(d_a_var, d_a_val, d_b_var, d_b_val, d_result_vars, &A));
    PG_TRY(check_columns(out));
    return launch<GD>(e, A, out, batch, gate_base, var_base, 0, nullptr, nullptr, stream, nullptr, values_only);
}

// the range widget (range_gate.hpp) on existing Variables: num_bits even, 2 .. 254 (checked by the caller).  An item of
// num_bits = 2 creates no Variable: its rows alone (EMIT_STRUCTURE: they are a function of the call), nothing when values_only.
static pg_status range_gate_common(pg_engine *e, const pg_variable *d_witness_var, const pg_scalar *d_witness_val, uint32_t num_bits,
                                   uint64_t batch, uint64_t gate_base, uint64_t var_base, uint64_t zero_var, const pg_columns *out,
                                   void *stream, bool values_only) {
    using GD = pg::RangeGateGD;
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    PG_TRY(check_u64s(d_witness_var, "d_witness_var"));
    PG_TRY(check_scalars(d_witness_val, "witness value array"));
    PG_TRY(check_columns(out));
    if ((batch + GD::W - 1) / GD::W > 0xffffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "batch too large for one call");
    pg::RangeGateArgs A;
    A.witness_vars = d_witness_var;
    A.witness = reinterpret_cast<const uint4 *>(d_witness_val);
    const pg::WidgetShape shape = pg::widget_shape(num_bits);
    A.k = shape.k; A.g = shape.g; A.pad = shape.pad;
    if (A.k == 1) {
        if (values_only) return PG_OK;
        return launch_mode<GD, pg::EMIT_STRUCTURE>(e, A, out, batch, gate_base, var_base, zero_var, stream);
    }
    if (values_only) return launch_mode<GD, pg::EMIT_VALUES>(e, A, out, batch, gate_base, var_base, zero_var, stream);
    return launch_mode<GD, pg::EMIT_ALL>(e, A, out, batch, gate_base, var_base, zero_var, stream);
}

// the interval gadget (interval_gate.hpp) on existing Variables: num_bits even, 2 .. 252, and the bounds' preconditions checked by the
// caller.  d_min / d_max: device arrays with a pair per item, or both NULL: *min, *max for the whole call.  Every item creates
// Variables (the two differences at least), so a refresh is never empty.
static pg_status interval_gate_common(pg_engine *e, const pg_variable *d_witness_var, const pg_scalar *d_witness_val, const pg::Fr &min,
                                      const pg::Fr &max, const pg_scalar *d_min, const pg_scalar *d_max, uint32_t num_bits, uint64_t batch,
                                      uint64_t gate_base, uint64_t var_base, uint64_t zero_var, const pg_columns *out, void *stream,
                                      bool values_only) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    PG_TRY(check_u64s(d_witness_var, "d_witness_var"));
    PG_TRY(check_scalars(d_witness_val, "witness value array"));
    PG_TRY(check_columns(out));
    if ((batch + 255) / 256 > 0xffffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "batch too large for one call");
    pg::IntervalGateArgs A;
    A.witness_vars = d_witness_var;
    A.witness = reinterpret_cast<const uint4 *>(d_witness_val);
    A.min = min;
    A.max = max;
    A.min_v = reinterpret_cast<const uint4 *>(d_min);
    A.max_v = reinterpret_cast<const uint4 *>(d_max);
    const pg::WidgetShape shape = pg::widget_shape(num_bits);
    A.k = shape.k; A.g = shape.g; A.pad = shape.pad;
    if (d_min) {
        PG_TRY(check_scalars(d_min, "d_min"));
        PG_TRY(check_scalars(d_max, "d_max"));
        using GD = pg::IntervalGateGD<true>;
        if (values_only) return launch_mode<GD, pg::EMIT_VALUES>(e, A, out, batch, gate_base, var_base, zero_var, stream);
        return launch_mode<GD, pg::EMIT_ALL>(e, A, out, batch, gate_base, var_base, zero_var, stream);
    }
    using GD = pg::IntervalGateGD<false>;
    if (values_only) return launch_mode<GD, pg::EMIT_VALUES>(e, A, out, batch, gate_base, var_base, zero_var, stream);
    return launch_mode<GD, pg::EMIT_ALL>(e, A, out, batch, gate_base, var_base, zero_var, stream);
}

// the comparison gadget (compare_gate.hpp) on two arrays of existing Variables: num_bits even, 2 .. 252 (checked by the caller).
// Every item creates Variables (z at least), so a refresh is never empty and there is no structure-only form.
static pg_status compare_gate_common(pg_engine *e, const pg_variable *d_x_var, const pg_scalar *d_x_val, const pg_variable *d_y_var,
                                     const pg_scalar *d_y_val, uint32_t num_bits, bool strict, uint64_t batch, uint64_t gate_base,
                                     uint64_t var_base, uint64_t zero_var, const pg_columns *out, pg_variable *d_result_vars, void *stream,
                                     bool values_only) {
    using GD = pg::CompareGateGD;
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    PG_TRY(check_u64s(d_x_var, "d_x_var"));
    PG_TRY(check_u64s(d_y_var, "d_y_var"));
    PG_TRY(check_scalars(d_x_val, "x value array"));
    PG_TRY(check_scalars(d_y_val, "y value array"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    PG_TRY(check_columns(out));
    if ((batch + GD::W - 1) / GD::W > 0xffffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "batch too large for one call");
    pg::CompareGateArgs A;
    A.x_vars = d_x_var;
    A.y_vars = d_y_var;
    A.x = reinterpret_cast<const uint4 *>(d_x_val);
    A.y = reinterpret_cast<const uint4 *>(d_y_val);
    pg::Fr pow = pg::fr_zero();  // 2^num_bits as a canonical integer
    pow.l[num_bits >> 6] = 1ull << (num_bits & 63);
    A.offset = pg::fr_sub(pg::fr_to_mont(pow), strict ? pg::fr_one() : pg::fr_zero());
    A.result_vars = d_result_vars;
    const pg::WidgetShape shape = pg::compare_shape(num_bits);
    A.k = shape.k; A.g = shape.g; A.pad = shape.pad;
    if (values_only) return launch_mode<GD, pg::EMIT_VALUES>(e, A, out, batch, gate_base, var_base, zero_var, stream);
    return launch_mode<GD, pg::EMIT_ALL>(e, A, out, batch, gate_base, var_base, zero_var, stream);
}

extern "C" {

pg_status pg_conditionally_select_zero_batch(pg_engine *e, const pg_variable *d_x_var, const pg_scalar *d_x_val,
                                             const pg_variable *d_select_var, const pg_scalar *d_select_val, uint64_t batch,
                                             uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                             pg_variable *d_result_vars, void *stream) {
    return two_input_common<pg::SelectZeroGD>(e, d_x_var, d_x_val, d_select_var, d_select_val, batch, gate_base, var_base, out,
                                              d_result_vars, stream, false);
}

pg_status pg_conditionally_select_one_batch(pg_engine *e, const pg_variable *d_y_var, const pg_scalar *d_y_val,
                                            const pg_variable *d_selector_var, const pg_scalar *d_selector_val,
                                            uint64_t batch, uint64_t gate_base, uint64_t var_base, const pg_columns *out,
                                            pg_variable *d_result_vars, void *stream) {
    return two_input_common<pg::SelectOneGD>(e, d_y_var, d_y_val, d_selector_var, d_selector_val, batch, gate_base, var_base, out,
                                             d_result_vars, stream, false);
}

pg_status pg_maybe_equal_batch(pg_engine *e, const pg_variable *d_a_var, const pg_scalar *d_a_val, const pg_variable *d_b_var,
                               const pg_scalar *d_b_val, uint64_t batch, uint64_t gate_base, uint64_t var_base,
                               const pg_columns *out, pg_variable *d_result_vars, void *stream) {
    return two_input_common<pg::MaybeEqualGD>(e, d_a_var, d_a_val, d_b_var, d_b_val, batch, gate_base, var_base, out, d_result_vars,
                                              stream, false);
}

pg_status pg_is_non_zero_plan(pg_engine *e, const pg_scalar *d_value_assigned, uint64_t batch, uint64_t *d_row_off,
                              uint64_t *d_var_off, uint8_t *d_err_mask, pg_layout *out, uint64_t *err_count, void *stream) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return error_plan(e, pg::is_non_zero_plan_kernel, d_value_assigned, batch, d_row_off, d_var_off, d_err_mask, out,
                      err_count, stream);
}

static pg_status is_non_zero_common(pg_engine *e, const pg_variable *d_var, const pg_scalar *d_value_assigned, uint64_t batch,
                                    const uint64_t *d_row_off, const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base,
                                    pg_variable zero_var, const pg_columns *out, void *stream, bool values_only) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    PG_TRY(check_u64s(d_var, "d_var"));
    PG_TRY(check_scalars(d_value_assigned, "d_value_assigned"));
    PG_TRY(check_u64s(d_row_off, "d_row_off"));
    PG_TRY(check_u64s(d_var_off, "d_var_off"));
    PG_TRY(check_columns(out));
    pg::ScalarArgs A{};
    A.a_var = d_var;
    A.b_val = reinterpret_cast<const uint4 *>(d_value_assigned);
    return launch<pg::IsNonZeroGD>(e, A, out, batch, gate_base, var_base, zero_var, d_row_off, d_var_off, stream, nullptr, values_only);
}

pg_status pg_is_non_zero_batch(pg_engine *e, const pg_variable *d_var, const pg_scalar *d_value_assigned, uint64_t batch,
                               const uint64_t *d_row_off, const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base,
                               pg_variable zero_var, const pg_columns *out, void *stream) {
    return is_non_zero_common(e, d_var, d_value_assigned, batch, d_row_off, d_var_off, gate_base, var_base, zero_var, out, stream, false);
}

pg_status pg_scalar_mix_plan(pg_engine *e, const pg_scalar *d_v, uint64_t batch, uint64_t *d_row_off, uint64_t *d_var_off,
                             uint8_t *d_err_mask, pg_layout *out, uint64_t *err_count, void *stream) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    return error_plan(e, pg::scalar_mix_plan_kernel, d_v, batch, d_row_off, d_var_off, d_err_mask, out, err_count, stream);
}

pg_status pg_scalar_mix_plan_async(pg_engine *e, const pg_scalar *d_v, uint64_t batch, uint64_t *d_row_off,
                                   uint64_t *d_var_off, uint8_t *d_err_mask, void *stream) {
    return error_plan(e, pg::scalar_mix_plan_kernel, d_v, batch, d_row_off, d_var_off, d_err_mask, nullptr, nullptr, stream);
}

static pg_status scalar_mix_common(pg_engine *e, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                                   const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, const uint64_t *d_row_off,
                                   const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base, pg_variable zero_var,
                                   const pg_columns *out, pg_variable *d_result_vars, void *stream, bool values_only) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return PG_OK;
    const pg_scalar *in[5] = {d_v, d_y, d_s, d_a, d_b};
    for (const pg_scalar *p : in) PG_TRY(check_scalars(p, "input array"));
    PG_TRY(check_u64s(d_row_off, "d_row_off"));
    PG_TRY(check_u64s(d_var_off, "d_var_off"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    PG_TRY(check_columns(out));
    pg::ScalarMixArgs A{};
    A.v = reinterpret_cast<const uint4 *>(d_v);
    A.y = reinterpret_cast<const uint4 *>(d_y);
    A.s = reinterpret_cast<const uint4 *>(d_s);
    A.a = reinterpret_cast<const uint4 *>(d_a);
    A.b = reinterpret_cast<const uint4 *>(d_b);
    A.result_vars = d_result_vars;
    return launch<pg::ScalarMixGD>(e, A, out, batch, gate_base, var_base, zero_var, d_row_off, d_var_off, stream, nullptr, values_only);
}

pg_status pg_scalar_mix_batch(pg_engine *e, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                              const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, const uint64_t *d_row_off,
                              const uint64_t *d_var_off, uint64_t gate_base, uint64_t var_base, pg_variable zero_var,
                              const pg_columns *out, pg_variable *d_result_vars, void *stream) {
    return scalar_mix_common(e, d_v, d_y, d_s, d_a, d_b, batch, d_row_off, d_var_off, gate_base, var_base, zero_var, out, d_result_vars,
                             stream, false);
}

static pg_status scalar_mix_planned_common(pg_engine *e, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                                           const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, uint64_t *d_row_off,
                                           uint64_t *d_var_off, uint8_t *d_err_mask, uint64_t gate_base, uint64_t var_base,
                                           pg_variable zero_var, const pg_columns *out, pg_variable *d_result_vars, void *stream,
                                           bool values_only) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (batch == 0) return pg_scalar_mix_plan_async(e, d_v, 0, d_row_off, d_var_off, d_err_mask, stream);
    const pg_scalar *in[5] = {d_v, d_y, d_s, d_a, d_b};
    for (const pg_scalar *p : in) PG_TRY(check_scalars(p, "input array"));
    PG_TRY(check_u64s(d_row_off, "d_row_off"));
    PG_TRY(check_u64s(d_var_off, "d_var_off"));
    PG_TRY(check_u64s(d_result_vars, "d_result_vars", true));
    PG_TRY(check_columns(out));
    PG_TRY(ensure_scratch(e, batch));
    pg::ScalarMixArgs A{};
    A.v = reinterpret_cast<const uint4 *>(d_v);
    A.y = reinterpret_cast<const uint4 *>(d_y);
    A.s = reinterpret_cast<const uint4 *>(d_s);
    A.a = reinterpret_cast<const uint4 *>(d_a);
    A.b = reinterpret_cast<const uint4 *>(d_b);
    A.result_vars = d_result_vars;
    pg::MixPlan P{};  // the call plans itself: the launch that inverts also makes the prefix sums (scalar_gadgets.hpp)
    P.agg = e->d_blk_agg.as<unsigned long long>();
    P.cap = (uint32_t)e->scratch_blocks;
    P.row_off = d_row_off;
    P.var_off = d_var_off;
    P.err_mask = d_err_mask;
    P.host = e->plan();
    return launch<pg::ScalarMixGD>(e, A, out, batch, gate_base, var_base, zero_var, d_row_off, d_var_off, stream, &P, values_only);
}

pg_status pg_scalar_mix_planned_batch(pg_engine *e, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                                      const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, uint64_t *d_row_off,
                                      uint64_t *d_var_off, uint8_t *d_err_mask, uint64_t gate_base, uint64_t var_base,
                                      pg_variable zero_var, const pg_columns *out, pg_variable *d_result_vars, void *stream) {
    return scalar_mix_planned_common(e, d_v, d_y, d_s, d_a, d_b, batch, d_row_off, d_var_off, d_err_mask, gate_base, var_base, zero_var,
                                     out, d_result_vars, stream, false);
}

pg_status pg_scalar_mix_values_batch(pg_engine *e, const pg_scalar *d_v, const pg_scalar *d_y, const pg_scalar *d_s,
                                     const pg_scalar *d_a, const pg_scalar *d_b, uint64_t batch, uint64_t *d_row_off,
                                     uint64_t *d_var_off, uint8_t *d_err_mask, pg_scalar *d_var_values, void *stream) {
    const pg_columns c = values_columns(d_var_values);
    return scalar_mix_planned_common(e, d_v, d_y, d_s, d_a, d_b, batch, d_row_off, d_var_off, d_err_mask, 0, 0, 0, &c, nullptr, stream,
                                     true);
}

#if defined(PG_MIX_STAMPS)  // timing build only: ticks (100 MHz) the fused mix's waves spent per phase since the last call; not in the header
extern "C" int pg_debug_mix_phases(unsigned long long out[12]) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pg::g_mix_phase_ticks), 12 * sizeof(unsigned long long)) != hipSuccess) return 1;
    const unsigned long long zero[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(pg::g_mix_phase_ticks), zero, sizeof zero) == hipSuccess ? 0 : 1;
}
#endif

pg_status pg_columns_slab_layout(uint64_t n_gates, uint64_t n_vars, uint64_t stride_bytes, uint64_t offsets[9], uint64_t *total_bytes) {
    if (!offsets || !total_bytes) return fail(PG_ERR_INVALID_ARGUMENT, "offsets / total_bytes is NULL");
    if (n_gates > (1ull << 40) || n_vars > (1ull << 40) || stride_bytes > (1ull << 44))
        return fail(PG_ERR_INVALID_ARGUMENT, "circuit or stride too large");
    constexpr uint64_t al = 2ull << 20;
    auto up = [](uint64_t x) { return (x + al - 1) / al * al; };
    const uint64_t ssz = up(n_gates * 32), wsz = up(n_gates * 8), vsz = up(n_vars * 32);
    const uint64_t stride = up(stride_bytes) > ssz ? up(stride_bytes) : ssz;
    for (int c = 0; c < 5; c++) offsets[c] = (uint64_t)c * stride;
    const uint64_t tail = 4 * stride + ssz;
    for (int c = 0; c < 3; c++) offsets[5 + c] = tail + (uint64_t)c * wsz;
    offsets[8] = tail + 3 * wsz;
    *total_bytes = tail + 3 * wsz + vsz;
    return PG_OK;
}

pg_status pg_fill_bytes(pg_engine *e, void *d_dst, uint64_t bytes, uint32_t streams, uint64_t pattern, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (!d_dst || !aligned(d_dst, 16) || (bytes & 15)) return fail(PG_ERR_INVALID_ARGUMENT, "dst/bytes not 16-byte aligned");
    if (bytes == 0) return PG_OK;
    PG_HIP_TRY(hipSetDevice(e->device));
    if (streams == 0) {  // short-lived workgroups, 8 KiB each, two resident per CU
        const uint64_t blocks = (bytes / 16 + pg::kFillOneshotUnits - 1) / pg::kFillOneshotUnits;
        if (blocks > 0x7fffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "buffer too large for one launch");
        PG_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(pg::fill_oneshot_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)pg::kFillOneshotLds));
        hipLaunchKernelGGL(pg::fill_oneshot_kernel, dim3((uint32_t)blocks), dim3(pg::kThreads), pg::kFillOneshotLds, static_cast<hipStream_t>(stream),
                           static_cast<uint4 *>(d_dst), bytes / 16, pattern);
        PG_HIP_TRY(hipGetLastError());
        return PG_OK;
    }
    if (streams < 1 || streams > 16) return fail(PG_ERR_INVALID_ARGUMENT, "streams must be in [0, 16]");
    uint64_t pieces = (bytes / 16 / streams + 65535) / 65536;
    const uint64_t cap = (uint64_t)e->num_cus * PG_GRID_BLOCKS_PER_CU;
    if (pieces < 1) pieces = 1;  // (fewer units than streams: the remainder loop of workgroup 0 writes them)
    hipLaunchKernelGGL(pg::fill_kernel, dim3(grid_cap(pieces, cap)), dim3(pg::kThreads), 0,
                       static_cast<hipStream_t>(stream), static_cast<uint4 *>(d_dst), bytes / 16, streams, pattern);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

pg_status pg_fill_columns(pg_engine *e, const pg_columns *out, uint64_t n_gates, uint64_t n_vars, uint64_t rows_per_tile,
                          uint64_t pattern, void *stream) {
    if (!e || !out) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_HIP_TRY(hipSetDevice(e->device));
    if (n_gates == 0 && n_vars == 0) return PG_OK;
    PG_TRY(check_columns(out));
    for (const void *p : {(const void *)out->w_l, (const void *)out->w_r, (const void *)out->w_o})
        if (!aligned(p, 16)) return fail(PG_ERR_INVALID_ARGUMENT, "pg_fill_columns: wire columns must be 16-byte aligned");
    if (rows_per_tile == 0) rows_per_tile = 32768;  // (about the emitters' tiles: 32 x 1031 rows of range_check, 16 x ~511 of max_bound)
    if (rows_per_tile % 8) return fail(PG_ERR_INVALID_ARGUMENT, "rows_per_tile must be a multiple of 8 (whole lines of every column)");
    uint64_t tiles = n_gates ? (n_gates + rows_per_tile - 1) / rows_per_tile : 1;
    if (tiles > 0xffffffffull) return fail(PG_ERR_INVALID_ARGUMENT, "too many tiles for one call");
    const uint64_t vars_per_tile = ((n_vars + tiles - 1) / tiles + 3) / 4 * 4;
    pg::EmitOut O = make_out(out, 0, 1, 0, 0, 0, nullptr, nullptr);
    O.tiles = (uint32_t)tiles;
    const uint64_t cap = (uint64_t)e->num_cus * PG_GRID_BLOCKS_PER_CU;
    hipLaunchKernelGGL(pg::fill_columns_kernel, dim3(grid_cap(tiles, cap)), dim3(pg::kThreads), 0,
                       static_cast<hipStream_t>(stream), O, n_gates, n_vars, rows_per_tile, vars_per_tile, pattern);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

}  // extern "C"

/* ---- the copy permutation as field elements (permutation_product.hpp) ------------------------------------------------- */
namespace {

// ROOT_OF_UNITY = 7^t, q - 1 = 2^32 t: canonical limbs (order exactly 2^32)
const uint64_t kRootOfUnity[4] = {0x3829971f439f0d2bull, 0xb63683508c2280b9ull, 0xd09b681922c813b4ull, 0x16a2a19edfe81f20ull};

pg::Fr domain_generator(uint32_t log2_n) {
    pg::Fr w = pg::fr_to_mont(pg::Fr{{kRootOfUnity[0], kRootOfUnity[1], kRootOfUnity[2], kRootOfUnity[3]}});
    for (uint32_t i = log2_n; i < 32; i++) w = pg::fr_mul(w, w);
    return w;
}

// the parts of e->d_pp beyond the domain's tables
struct PpScratch {
    uint32_t *flags;
    uint4 *tile_prod, *tile_carry, *den;  // the product's own arrays (pg_sigma_evaluations has none: tiles = den_units = 0)
};

// the call's domain: padded_n a power of two <= 2^32; scratch laid out as flags (1 unit) | lo | hi | 2 tiles of tile products |
// 2 tiles of carries | den_units of denominators (16-byte units); the tables built with multipliers c[j] on `st`
pg_status pp_prepare(pg_engine *e, uint64_t padded_n, const pg_scalar *omega, const pg::Fr c[4], uint64_t tiles, uint64_t den_units,
                     hipStream_t st, pg::PpDomain &D, PpScratch &W) {
    if (padded_n == 0 || (padded_n & (padded_n - 1)) || padded_n > (1ull << 32))
        return fail(PG_ERR_INVALID_ARGUMENT, "padded_n must be a power of two <= 2^32");
    PG_TRY(check_field(omega, "omega"));
    D.padded_n = padded_n;
    D.m = 0;
    while ((1ull << D.m) < padded_n) D.m++;
    D.L = D.m < pg::kPpLoBitsMax ? D.m : pg::kPpLoBitsMax;
    D.H = padded_n >> D.L;
    uint4 *lo, *hi;
    PG_TRY(e->d_pp.carve(16, [&](Carve cv) {
        W.flags = cv.take<uint32_t>(1);
        lo = cv.take<uint4>(2 * (1ull << D.L));
        hi = cv.take<uint4>(8 * D.H);
        W.tile_prod = cv.take<uint4>(2 * tiles);
        W.tile_carry = cv.take<uint4>(2 * tiles);
        W.den = cv.take<uint4>(den_units);
        return cv.bytes();
    }));
    D.lo = lo;
    D.hi = hi;
    pg::PpPowers P;
    fill_squares(P.pw, to_fr(omega));
    for (int j = 0; j < 4; j++) P.c[j] = c[j];
    PG_HIP_TRY(hipMemsetAsync(W.flags, 0, sizeof(uint32_t), st));
    const uint64_t entries = (1ull << D.L) + D.H, want = (entries + pg::kThreads - 1) / pg::kThreads, cap = (uint64_t)e->num_cus * 8;
    hipLaunchKernelGGL(pg::pp_tables_kernel, dim3(grid_cap(want, cap)), dim3(pg::kThreads), 0, st, P, D.L, D.H, 4u, lo, hi);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

// the flags after the call's launches (synchronises)
pg_status pp_finish(pg_engine *e, uint32_t *flags, hipStream_t st) {
    uint32_t h = 0;
    PG_HIP_TRY(hipGetLastError());
    PG_HIP_TRY(hipMemcpyAsync(&h, flags, sizeof h, hipMemcpyDeviceToHost, st));
    PG_HIP_TRY(hipStreamSynchronize(st));
    (void)e;
    if (h & pg::kPpFlagBadSigma) return fail(PG_ERR_INVALID_ARGUMENT, "a sigma entry is >= 4 * padded_n");
    if (h & pg::kPpFlagZeroDen) return fail(PG_ERR_NON_EXISTING_INVERSE, "a denominator w + beta * sigma + gamma is zero");
    return PG_OK;
}

}  // namespace

extern "C" {

pg_status pg_domain_generator(uint32_t log2_n, pg_scalar *out) {
    if (!out) return fail(PG_ERR_INVALID_ARGUMENT, "out is NULL");
    if (log2_n > 32) return fail(PG_ERR_INVALID_ARGUMENT, "log2_n > 32: the scalar field has no such subgroup");
    from_fr(domain_generator(log2_n), out);
    return PG_OK;
}

pg_status pg_sigma_evaluations(pg_engine *e, const uint64_t *d_sigma, uint64_t padded_n, const pg_scalar *omega, const pg_scalar k[4],
                               pg_scalar *d_out, void *stream) {
    if (!e || !k) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_u64s(d_sigma, "d_sigma"));
    PG_TRY(check_scalars(d_out, "d_out"));
    pg::Fr c[4];
    for (int j = 0; j < 4; j++) {
        PG_TRY(check_field(&k[j], "k[j]"));
        c[j] = to_fr(&k[j]);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    pg::PpDomain D;
    PpScratch W;
    PG_TRY(pp_prepare(e, padded_n, omega, c, 0, 0, st, D, W));
    const uint64_t want = (4 * padded_n + pg::kThreads - 1) / pg::kThreads, cap = (uint64_t)e->num_cus * 32;
    hipLaunchKernelGGL(pg::pp_sigma_eval_kernel, dim3(grid_cap(want, cap)), dim3(pg::kThreads), 0, st, D, d_sigma,
                       reinterpret_cast<uint4 *>(d_out), W.flags);
    return pp_finish(e, W.flags, st);
}

pg_status pg_permutation_product(pg_engine *e, uint64_t padded_n, const pg_scalar *const d_wire_values[4], uint64_t n_values,
                                 const uint64_t *d_sigma, const pg_scalar *omega, const pg_scalar k[4], const pg_scalar *beta,
                                 const pg_scalar *gamma, pg_scalar *d_z, pg_scalar *d_wrap, void *stream) {
    if (!e || !k || (n_values && !d_wire_values)) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_values > padded_n) return fail(PG_ERR_INVALID_ARGUMENT, "n_values > padded_n");
    PG_TRY(check_u64s(d_sigma, "d_sigma"));
    PG_TRY(check_scalars(d_z, "d_z"));
    PG_TRY(check_scalars(d_wrap, "d_wrap"));
    PG_TRY(check_field(beta, "beta"));
    PG_TRY(check_field(gamma, "gamma"));
    pg::PpProduct A{};
    for (int j = 0; j < 4 && n_values; j++) {
        PG_TRY(check_scalars(d_wire_values[j], "d_wire_values[j]"));
        A.w[j] = reinterpret_cast<const uint4 *>(d_wire_values[j]);
    }
    pg::Fr c[4];
    for (int j = 0; j < 4; j++) {
        PG_TRY(check_field(&k[j], "k[j]"));
        c[j] = pg::fr_mul(to_fr(beta), to_fr(&k[j]));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    const uint64_t tiles = (padded_n + pg::kPpTile - 1) / pg::kPpTile;
    // launch 1 loops over the tiles with the workgroups that fit at once (two per CU: 178 registers), each owning a slab of denominators
    const uint64_t grid = grid_cap(tiles, (uint64_t)e->num_cus * 2);
    PpScratch W;
    PG_TRY(pp_prepare(e, padded_n, omega, c, tiles, 2 * grid * pg::kPpTile, st, A.D, W));
    A.n_values = n_values;
    A.sigma = d_sigma;
    A.gamma = to_fr(gamma);
    A.z = reinterpret_cast<uint4 *>(d_z);
    A.wrap = reinterpret_cast<uint4 *>(d_wrap);
    A.tile_prod = W.tile_prod;
    A.tile_carry = W.tile_carry;
    A.den = W.den;
    A.tiles = tiles;
    A.flags = W.flags;
    hipLaunchKernelGGL(pg::pp_ratio_kernel, dim3((uint32_t)grid), dim3(pg::kThreads), 0, st, A);
    hipLaunchKernelGGL(pg::pp_carry_kernel, dim3(1), dim3(pg::kThreads), 0, st, A);
    hipLaunchKernelGGL(pg::pp_scan_kernel, dim3((uint32_t)tiles), dim3(pg::kThreads), 0, st, A);
    return pp_finish(e, W.flags, st);
}

}  // extern "C"

/* ---- NTTs over the scalar field (ntt.hpp) -------------------------------------------------------------------------------- */
namespace {

// room for the tables of base^x, x < 2^m: lo (2^L entries) | hi (H entries), two 16-byte units an entry
struct NttTableAt {
    uint4 *lo, *hi;
    uint32_t L;
};
NttTableAt ntt_table_part(Carve &cv, uint32_t m) {
    const uint32_t L = m < pg::kNttTileBits ? m : pg::kNttTileBits;
    uint4 *lo = cv.take<uint4>(2 * (1ull << L));
    return NttTableAt{lo, cv.take<uint4>(2 * ((1ull << m) >> L)), L};
}

// the tables built at `at` (of ntt_table_part, for the same m) on `st`: lo[e] = base^e, hi[h] = c base^(h 2^L)
pg::NttTable ntt_table(const pg::Fr &base, const pg::Fr &c, uint32_t m, const NttTableAt &at, int num_cus, hipStream_t st) {
    const uint64_t H = (1ull << m) >> at.L;
    pg::PpPowers P{};
    fill_squares(P.pw, base);
    P.c[0] = c;
    const uint64_t entries = (1ull << at.L) + H, want = (entries + pg::kThreads - 1) / pg::kThreads, cap = (uint64_t)num_cus * 8;
    hipLaunchKernelGGL(pg::pp_tables_kernel, dim3(grid_cap(want, cap)), dim3(pg::kThreads), 0, st, P, at.L, H, 1u, at.lo, at.hi);
    return pg::NttTable{at.lo, at.hi, at.L};
}

// enqueue the transform of pg_ntt (its arguments checked, `st` entered) on the n_cols columns of `data`; src non-NULL: the columns
// are read from src (same stride) and written to data (out of place, in the first pass)
pg_status ntt_enqueue(pg_engine *e, uint4 *data, const uint4 *src, uint64_t n_cols, uint64_t col_stride, uint32_t m, bool coset,
                      bool inverse, const pg::Fr &w, const pg::Fr &g, hipStream_t st) {
    const uint64_t n = 1ull << m;
    NttTableAt w_at{}, g_at{};
    PG_TRY(e->d_ntt.carve(16, [&](Carve cv) {
        w_at = ntt_table_part(cv, m);
        if (coset) g_at = ntt_table_part(cv, m);
        return cv.bytes();
    }));
    const pg::Fr n_inv = pg::fr_invert_or_zero(pg::fr_from_u64(n));  // (n = 2^32 fits: fr_from_u64 takes the full 64 bits)
    pg::NttPass P{};
    P.data = data;
    P.n_cols = n_cols;
    P.stride = col_stride;
    P.m = m;
    P.w = ntt_table(inverse ? pg::fr_invert_or_zero(w) : w, pg::fr_one(), m, w_at, e->num_cus, st);
    pg::NttTable none{nullptr, nullptr, 0}, gt = none;
    if (coset) gt = inverse ? ntt_table(pg::fr_invert_or_zero(g), n_inv, m, g_at, e->num_cus, st)
                            : ntt_table(g, pg::fr_one(), m, g_at, e->num_cus, st);
    P.scale = n_inv;
    P.use_scale = inverse && !coset;
    const uint64_t resident = (uint64_t)e->num_cus * 3;  // (48 KiB of LDS per pass workgroup: three per CU)
    auto pass = [&](uint32_t bp, uint32_t k, uint32_t cb, bool first, bool last) {
        P.bp = bp;
        P.k = k;
        P.cb = cb;
        P.twiddle = !last;
        P.natural = m <= pg::kNttTileBits;
        P.src = first ? src : nullptr;
        P.pre = first && coset && !inverse ? gt : none;
        P.post = P.natural && coset && inverse ? gt : none;
        const uint64_t tiles = n_cols << (m - k - cb);
        hipLaunchKernelGGL(pg::ntt_pass_kernel, dim3(grid_cap(tiles, resident)), dim3(pg::kThreads), 0, st, P);
    };
    if (m <= pg::kNttTileBits) {
        pass(m, m, 0, true, true);
    } else {
        // the top m - 10 bits in passes of at most 2^7 points per column, as even as possible; then the last 2^10
        const uint32_t top = m - pg::kNttTileBits, np = (top + pg::kNttStridedBits - 1) / pg::kNttStridedBits;
        uint32_t bp = m;
        for (uint32_t p = 0; p < np; p++) {
            const uint32_t k = top / np + (p < top % np ? 1 : 0);
            pass(bp, k, pg::kNttTileBits - k, p == 0, false);
            bp -= k;
        }
        pass(bp, pg::kNttTileBits, 0, false, true);
        P.src = nullptr;
        P.pre = none;
        P.post = coset && inverse ? gt : none;
        const uint64_t tiles = n_cols << (m - 2 * pg::kNttRevBits), cap = (uint64_t)e->num_cus * 2;  // (66 KiB of LDS: two per CU)
        hipLaunchKernelGGL(pg::ntt_reverse_kernel, dim3(grid_cap(tiles, cap)), dim3(pg::kThreads), 0, st, P);
    }
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

}  // namespace

extern "C" {

pg_status pg_ntt(pg_engine *e, pg_scalar *d_data, uint64_t n_cols, uint64_t col_stride, uint32_t log2_n, uint32_t kind,
                 const pg_scalar *omega, const pg_scalar *coset_gen, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_scalars(d_data, "d_data"));
    if (log2_n > 32) return fail(PG_ERR_INVALID_ARGUMENT, "log2_n > 32: the scalar field has no such subgroup");
    if (kind > PG_NTT_COSET_INVERSE) return fail(PG_ERR_INVALID_ARGUMENT, "unknown kind");
    const uint32_t m = log2_n;
    const uint64_t n = 1ull << m;
    PG_TRY(check_strided_columns(n, n_cols, col_stride));
    PG_TRY(check_field(omega, "omega"));
    pg::Fr w = to_fr(omega), x = w;
    for (uint32_t i = 1; i < m; i++) x = pg::fr_mul(x, x);
    if (!pg::fr_eq(x, m ? pg::fr_neg_one() : pg::fr_one()))
        return fail(PG_ERR_INVALID_ARGUMENT, "omega is not a primitive 2^log2_n-th root of unity");
    const bool coset = kind == PG_NTT_COSET_FORWARD || kind == PG_NTT_COSET_INVERSE;
    const bool inverse = kind == PG_NTT_INVERSE || kind == PG_NTT_COSET_INVERSE;
    pg::Fr g = pg::fr_one();
    if (coset) {
        PG_TRY(check_field(coset_gen, "coset_gen"));
        g = to_fr(coset_gen);
        if (pg::fr_is_zero(g)) return fail(PG_ERR_INVALID_ARGUMENT, "coset_gen is zero");
    }
    if (n_cols == 0) return PG_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    return ntt_enqueue(e, reinterpret_cast<uint4 *>(d_data), nullptr, n_cols, col_stride, m, coset, inverse, w, g, st);
}

}  // extern "C"

/* ---- the quotient polynomial and evaluations at a point (quotient.hpp) -------------------------------------------------- */
namespace {

pg::Fr fr_sqr_times(pg::Fr x, uint32_t times) {  // x^(2^times)
    for (uint32_t i = 0; i < times; i++) x = pg::fr_mul(x, x);
    return x;
}

// workgroups for `items` work items of kThreads lanes, at most per_cu per CU (the kernels loop over the rest)
uint32_t grid_of(const pg_engine *e, uint64_t items, uint64_t per_cu) {
    const uint64_t want = (items + pg::kThreads - 1) / pg::kThreads, cap = (uint64_t)e->num_cus * per_cu;
    return (uint32_t)(want < cap ? (want ? want : 1) : cap);
}

template <int OP>
void quotient_step(const pg_engine *e, const pg::QuotientChunk &A, hipStream_t st) {
    const uint32_t grid = OP == pg::QS_PERM_NUM ? grid_of(e, (A.n + pg::kQRowsPerLane - 1) / pg::kQRowsPerLane, 8) : grid_of(e, A.n, 8);
    hipLaunchKernelGGL(pg::quotient_step_kernel<OP>, dim3(grid), dim3(pg::kThreads), 0, st, A);
}

// pg_quotient (blinded = false: today's launches, nothing else) and pg_quotient_blinded (w[j] of n + 2 rows, z of n + 3, d_t of
// 4n + 8: QS_BLIND after each chunk's five wire / z transforms and quotient_top_kernel after the combine)
pg_status quotient_enqueue(pg_engine *e, uint32_t log2_n, const pg_quotient_polys *p, const pg_scalar *alpha, const pg_scalar *beta,
                           const pg_scalar *gamma, const pg_scalar *omega_4n, const pg_scalar k[4], const pg_scalar *coset_gen,
                           pg_scalar *d_t, pg_scalar *d_scratch, void *stream, bool blinded, const pg_scalar *q_range = nullptr) {
    if (!e || !p || !k) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (log2_n > 30) return fail(PG_ERR_INVALID_ARGUMENT, "log2_n > 30");
    if (blinded && log2_n < 3) return fail(PG_ERR_INVALID_ARGUMENT, "log2_n < 3: the blinders' rows would meet the top rows");
    const uint32_t m = log2_n;
    const uint64_t n = 1ull << m, col_bytes = n * sizeof(pg_scalar);
    // the inputs in the order the chunks consume them; pi and q_range (pg_quotient_range alone) may be NULL
    const pg_scalar *in[18] = {p->w[0], p->w[1], p->w[2], p->w[3], p->z, p->q_m, p->q_l, p->q_r, p->q_o, p->q_4,
                               p->q_c, p->q_arith, p->sigma[0], p->sigma[1], p->sigma[2], p->sigma[3], p->pi, q_range};
    for (int i = 0; i < 16; i++) PG_TRY(check_scalars(in[i], "an input polynomial"));
    if (p->pi) PG_TRY(check_scalars(p->pi, "pi"));
    if (q_range) PG_TRY(check_scalars(q_range, "q_range"));
    PG_TRY(check_scalars(d_t, "d_t"));
    PG_TRY(check_scalars(d_scratch, "d_scratch"));
    PG_TRY(check_field(alpha, "alpha"));
    PG_TRY(check_field(beta, "beta"));
    PG_TRY(check_field(gamma, "gamma"));
    PG_TRY(check_field(omega_4n, "omega_4n"));
    PG_TRY(check_field(coset_gen, "coset_gen"));
    for (int j = 0; j < 4; j++) PG_TRY(check_field(&k[j], "k[j]"));
    const pg::Fr zeta = to_fr(omega_4n), g = to_fr(coset_gen);
    if (!pg::fr_eq(fr_sqr_times(zeta, m + 1), pg::fr_neg_one()))
        return fail(PG_ERR_INVALID_ARGUMENT, "omega_4n is not a primitive 4n-th root of unity");
    if (pg::fr_is_zero(g) || pg::fr_eq(fr_sqr_times(g, m + 2), pg::fr_one()))
        return fail(PG_ERR_INVALID_ARGUMENT, "coset_gen is zero or coset_gen^(4n) = 1: the coset meets H");
    const uint64_t t_bytes = 4 * col_bytes + (blinded ? 8 * sizeof(pg_scalar) : 0), s_bytes = PG_QUOTIENT_SCRATCH_COLS * col_bytes;
    if (overlaps(d_t, t_bytes, d_scratch, s_bytes)) return fail(PG_ERR_INVALID_ARGUMENT, "d_t overlaps d_scratch");
    for (int i = 0; i < 18; i++) {
        const pg_scalar *x = in[i];
        const uint64_t x_bytes = col_bytes + (blinded && i < 5 ? (i < 4 ? 2 : 3) * sizeof(pg_scalar) : 0);  // the tails of w[j] and z
        if (x && (overlaps(d_t, t_bytes, x, x_bytes) || overlaps(d_scratch, s_bytes, x, x_bytes)))
            return fail(PG_ERR_INVALID_ARGUMENT, "d_t or d_scratch overlaps an input polynomial");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    NttTableAt x_at{};  // the chunk's points x
    PG_TRY(e->d_quot.carve(16, [&](Carve cv) {
        x_at = ntt_table_part(cv, m);
        return cv.bytes();
    }));
    const pg::Fr omega = fr_sqr_times(zeta, 2), zeta_n = fr_sqr_times(zeta, m), g_n = fr_sqr_times(g, m);
    uint4 *T = reinterpret_cast<uint4 *>(d_t), *S = reinterpret_cast<uint4 *>(d_scratch);
    pg::QuotientChunk A{};
    A.s = S;
    A.n = n;
    A.has_pi = p->pi != nullptr;
    A.alpha = to_fr(alpha);
    A.beta = to_fr(beta);
    A.gamma = to_fr(gamma);
    for (int j = 0; j < 4; j++) A.beta_k[j] = pg::fr_mul(A.beta, to_fr(&k[j]));
    A.n_fr = pg::fr_from_u64(n);
    const pg::Fr alpha2 = pg::fr_mul(A.alpha, A.alpha);
    pg::QuotientRange Rg{};
    Rg.alpha[0] = pg::fr_mul(alpha2, A.alpha);
    Rg.alpha[1] = pg::fr_mul(Rg.alpha[0], A.alpha);
    Rg.alpha[2] = pg::fr_mul(Rg.alpha[1], A.alpha);
    if (blinded)
        for (int i = 0; i < 5; i++) A.tail[i] = reinterpret_cast<const uint4 *>(in[i]) + 2 * n;
    pg::Fr g_j = g, zeta_jn = pg::fr_one();  // g zeta^j, zeta^(jn)
    for (uint32_t j = 0; j < 4; j++) {
        // coset-forward transform of input i into scratch column c, with generator g_j
        auto fwd = [&](int i, uint32_t c) {
            return ntt_enqueue(e, S + 2 * c * n, reinterpret_cast<const uint4 *>(in[i]), 1, n, m, true, false, omega, g_j, st);
        };
        const pg::Fr c_j = pg::fr_sub(pg::fr_mul(g_n, zeta_jn), pg::fr_one());  // x^n - 1 on the chunk
        A.t = T + 2 * j * n;
        A.x = ntt_table(omega, g_j, m, x_at, e->num_cus, st);
        A.alpha2_c = pg::fr_mul(alpha2, c_j);
        A.c_inv = pg::fr_invert_or_zero(c_j);
        for (int i = 0; i < 5; i++) PG_TRY(fwd(i, (uint32_t)i));  // a, b, c, d, z: resident for the chunk
        if (blinded) {  // QS_BLIND
            A.xn = pg::fr_mul(g_n, zeta_jn);
            hipLaunchKernelGGL(pg::quotient_blind_kernel, dim3(grid_of(e, n, 8)), dim3(pg::kThreads), 0, st, A);
        }
        quotient_step<pg::QS_PERM_NUM>(e, A, st);
        PG_TRY(fwd(5, 5)); PG_TRY(fwd(6, 6)); PG_TRY(fwd(7, 7));  // q_m, q_l, q_r
        quotient_step<pg::QS_GATE1>(e, A, st);
        PG_TRY(fwd(8, 6)); PG_TRY(fwd(9, 7));  // q_o, q_4
        quotient_step<pg::QS_GATE2>(e, A, st);
        PG_TRY(fwd(10, 6)); PG_TRY(fwd(11, 7));  // q_c, q_arith
        quotient_step<pg::QS_GATE3>(e, A, st);
        if (q_range) {  // the range widget's term: q_range through column 5, which is free until QS_PERM1's inputs arrive
            PG_TRY(fwd(17, 5));
            hipLaunchKernelGGL(pg::quotient_range_kernel, dim3(grid_of(e, n, 8)), dim3(pg::kThreads), 0, st, A, Rg);
        }
        if (p->pi) PG_TRY(fwd(16, 5));
        PG_TRY(fwd(12, 6)); PG_TRY(fwd(13, 7));  // sigma_1, sigma_2
        quotient_step<pg::QS_PERM1>(e, A, st);
        PG_TRY(fwd(14, 5)); PG_TRY(fwd(15, 7));  // sigma_3, sigma_4
        quotient_step<pg::QS_PERM2>(e, A, st);
        // chunk j of t, in place: sum_k1 t[k0 + n k1] g_j^(n k1)
        PG_TRY(ntt_enqueue(e, A.t, nullptr, 1, n, m, true, true, omega, g_j, st));
        g_j = pg::fr_mul(g_j, zeta);
        zeta_jn = pg::fr_mul(zeta_jn, zeta_n);
    }
    pg::QuotientCombine Cb{};
    Cb.t = T;
    Cb.n = n;
    Cb.iota = pg::fr_invert_or_zero(zeta_n);
    const pg::Fr g_n_inv = pg::fr_invert_or_zero(g_n);
    Cb.scale[0] = pg::fr_invert_or_zero(pg::fr_from_u64(4));
    for (int j = 1; j < 4; j++) Cb.scale[j] = pg::fr_mul(Cb.scale[j - 1], g_n_inv);
    hipLaunchKernelGGL(pg::quotient_combine_kernel, dim3(grid_of(e, n, 8)), dim3(pg::kThreads), 0, st, Cb);
    if (blinded) {
        pg::QuotientTop Tp{};
        for (int j = 0; j < 4; j++) {
            Tp.w[j] = reinterpret_cast<const uint4 *>(p->w[j]);
            Tp.sigma[j] = reinterpret_cast<const uint4 *>(p->sigma[j]);
        }
        Tp.z = reinterpret_cast<const uint4 *>(p->z);
        Tp.t = T;
        Tp.n = n;
        Tp.alpha = A.alpha;
        Tp.beta = A.beta;
        Tp.g4n = fr_sqr_times(g_n, 2);
        // omega^(n + 2 - d) = omega^2, omega, 1, omega^-1, ..., omega^-4
        const pg::Fr omega_inv = pg::fr_invert_or_zero(omega);
        Tp.zw[2] = pg::fr_one();
        Tp.zw[1] = omega;
        Tp.zw[0] = pg::fr_mul(omega, omega);
        for (uint32_t d = 3; d < pg::kQTop; d++) Tp.zw[d] = pg::fr_mul(Tp.zw[d - 1], omega_inv);
        hipLaunchKernelGGL(pg::quotient_top_kernel, dim3(1), dim3(pg::kQTopLanes), 0, st, Tp);
        if (q_range) {
            pg::QuotientRangeTop Rt{};
            for (int j = 0; j < 3; j++) Rt.w[j] = reinterpret_cast<const uint4 *>(p->w[j]);
            Rt.q_range = reinterpret_cast<const uint4 *>(q_range);
            Rt.t = T;
            Rt.n = n;
            for (int j = 0; j < 3; j++) Rt.alpha[j] = Rg.alpha[j];
            Rt.g4n = Tp.g4n;
            // omega^(n + 1 - d) = omega, 1, omega^-1, omega^-2
            Rt.aw[0] = omega;
            Rt.aw[1] = pg::fr_one();
            Rt.aw[2] = omega_inv;
            Rt.aw[3] = pg::fr_mul(omega_inv, omega_inv);
            hipLaunchKernelGGL(pg::quotient_range_top_kernel, dim3(1), dim3(pg::kQTopLanes), 0, st, Rt);
        }
    }
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

}  // namespace

extern "C" {

pg_status pg_quotient(pg_engine *e, uint32_t log2_n, const pg_quotient_polys *p, const pg_scalar *alpha, const pg_scalar *beta,
                      const pg_scalar *gamma, const pg_scalar *omega_4n, const pg_scalar k[4], const pg_scalar *coset_gen,
                      pg_scalar *d_t, pg_scalar *d_scratch, void *stream) {
    return quotient_enqueue(e, log2_n, p, alpha, beta, gamma, omega_4n, k, coset_gen, d_t, d_scratch, stream, false);
}

pg_status pg_quotient_blinded(pg_engine *e, uint32_t log2_n, const pg_quotient_polys *p, const pg_scalar *alpha,
                              const pg_scalar *beta, const pg_scalar *gamma, const pg_scalar *omega_4n, const pg_scalar k[4],
                              const pg_scalar *coset_gen, pg_scalar *d_t, pg_scalar *d_scratch, void *stream) {
    return quotient_enqueue(e, log2_n, p, alpha, beta, gamma, omega_4n, k, coset_gen, d_t, d_scratch, stream, true);
}

pg_status pg_quotient_range(pg_engine *e, uint32_t log2_n, const pg_quotient_polys *p, const pg_scalar *d_q_range, int blinded,
                            const pg_scalar *alpha, const pg_scalar *beta, const pg_scalar *gamma, const pg_scalar *omega_4n,
                            const pg_scalar k[4], const pg_scalar *coset_gen, pg_scalar *d_t, pg_scalar *d_scratch, void *stream) {
    return quotient_enqueue(e, log2_n, p, alpha, beta, gamma, omega_4n, k, coset_gen, d_t, d_scratch, stream, blinded != 0, d_q_range);
}

pg_status pg_poly_evaluate(pg_engine *e, const pg_scalar *d_coeffs, uint64_t n_cols, uint64_t col_stride, uint64_t n,
                           const pg_scalar *point, pg_scalar *d_out, void *stream) {
    if (!e) return fail(PG_ERR_INVALID_ARGUMENT, "NULL argument");
    PG_TRY(check_scalars(d_coeffs, "d_coeffs"));
    PG_TRY(check_scalars(d_out, "d_out"));
    PG_TRY(check_field(point, "point"));
    if (n == 0 || n > (1ull << 32)) return fail(PG_ERR_INVALID_ARGUMENT, "n must be in [1, 2^32]");
    PG_TRY(check_strided_columns(n, n_cols, col_stride));
    if (n_cols == 0) return PG_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PG_TRY(enter_stream(e, st));
    StreamScope scope{e, st};
    pg::PolyEval A{};
    A.segs = (n + pg::kEvalSeg - 1) / pg::kEvalSeg;
    uint4 *lane, *seg_lo, *seg;
    PG_TRY(e->d_eval.carve(16, [&](Carve cv) {
        lane = cv.take<uint4>(2 * 256);
        seg_lo = cv.take<uint4>(2);  // ONE entry directly in front of seg: the second pp_tables launch writes its lo table of 2^0 entries here
        seg = cv.take<uint4>(2 * A.segs);
        A.partial = cv.take<uint4>(2 * n_cols * A.segs);
        return cv.bytes();
    }));
    A.c = reinterpret_cast<const uint4 *>(d_coeffs);
    A.n_cols = n_cols;
    A.stride = col_stride;
    A.n = n;
    A.x_lane = lane;
    A.x_seg = seg;
    A.out = reinterpret_cast<uint4 *>(d_out);
    const pg::Fr x = to_fr(point);
    A.x256 = fr_sqr_times(x, 8);
    // lane[t] = x^t (t < 256); seg[s] = x^(s kEvalSeg) (s < segs)
    pg::PpPowers P{};
    fill_squares(P.pw, x);
    P.c[0] = pg::fr_one();
    hipLaunchKernelGGL(pg::pp_tables_kernel, dim3(1), dim3(pg::kThreads), 0, st, P, 8u, (uint64_t)0, 1u, lane, lane);
    static_assert(pg::kEvalSeg == (1u << 14), "x^kEvalSeg");
    fill_squares(P.pw, fr_sqr_times(x, 14));
    hipLaunchKernelGGL(pg::pp_tables_kernel, dim3(grid_of(e, A.segs + 1, 8)), dim3(pg::kThreads), 0, st, P, 0u, A.segs, 1u, seg_lo, seg);
    const uint64_t cap = (uint64_t)e->num_cus * 8;
    hipLaunchKernelGGL(pg::poly_eval_kernel, dim3(grid_cap(n_cols * A.segs, cap)), dim3(pg::kThreads), 0, st, A);
    hipLaunchKernelGGL(pg::poly_eval_reduce_kernel, dim3(grid_cap(n_cols, cap)), dim3(pg::kThreads), 0, st, A);
    PG_HIP_TRY(hipGetLastError());
    return PG_OK;
}

}  // extern "C"

#include "capi_composer.inc"
#include "capi_dist.inc"
#include "capi_msm.inc"
#include "capi_msm_small.inc"
#include "capi_open.inc"
#include "capi_pairing.inc"
#include "capi_codec.inc"
#include "capi_sides.inc"
