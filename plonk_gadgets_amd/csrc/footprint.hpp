// footprint.hpp -- what a batched append leaves behind for the f-rows (PermSeg), what every kind of footprint weighs per item
// (kind_rows, kind_vars, kind_foreign) and which kernel writes a footprint's rows: perm_route for pg_composer_permutation,
// mat_route for pg_composer_materialize.  Each consumer classifies a footprint ONCE and switches on the answer; nothing else in
// the library decides by wire_kind / row_off / tail / wire_n.  No HIP in here: a plain host compiler sees this header alone
// (tests/cpp/footprint_host.cpp, g++), the device code through permutation.hpp.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PG_FOOTPRINT_HD __host__ __device__
#else
#define PG_FOOTPRINT_HD
#endif

namespace pg {

// footprint of a batched call: `items` items, each owning a run of rows and a run of Variables it created itself.
// Uniform calls: L rows / V Variables per item.  Ragged calls (per-item public bounds, is_non_zero items that stop at
// their error): row_off / var_off are the call's exclusive prefix sums (items + 1 entries, relative to the bases) and
// L, V the largest item.  `group` consecutive items are linked by one workgroup as if they were one item.
struct PermSeg {
    uint64_t gate_base, gate_end, var_base, var_end;
    uint32_t L, V;
    uint64_t items;
    const uint64_t *row_off, *var_off;
    uint32_t group;
    // The call's wires in closed form (0: not known -- read the wire columns): the ladder gadgets' rows reference the item's own
    // Variables at offsets that are a function of the row and the ladder length alone (range_gadgets.hpp, bound_wire_offsets:
    // what the emitter wrote them from), so whoever needs the Variables of a row -- the wire-value columns of
    // pg_composer_materialize -- can compute them instead of reading 24 bytes per row back.
    uint32_t wire_kind, wire_n;
    // perm_ladder_kernel: the segment's slots on the sparse list -- ladder_foreign_per_item(wire_kind) per item, in closed form (set by
    // pg_composer_permutation for the pass it launches)
    uint64_t sparse_base;
    // Rows behind every item's own that hold its RESULT Variable on all three wires (constrain_to_constant / boolean_gate on the result:
    // the loop of the reference's tests, recorded call by call and flushed as one launch -- capi_composer.inc, flush): they count as
    // the item's rows (L includes them), their wires and their place in the result's cycle are closed forms like the others.  Kinds that
    // allocate their witness only.
    uint32_t tail;
    // perm_ladder_kernel<true> (per-item bounds): the item that holds the first row of every piece of kPermLadderRows rows (set by
    // pg_composer_permutation for the pass it launches; perm_piece_items_kernel fills it from the call's prefix sums)
    const uint32_t *piece_item;
};
enum : uint32_t { WIRES_UNKNOWN = 0, WIRES_RANGE_CHECK = 1, WIRES_MAX_BOUND = 2, WIRES_RANGE_CHECK_ALLOCATED = 3, WIRES_MAX_BOUND_ALLOCATED = 4,
                  WIRES_DECOMPOSITION = 5,
                  WIRES_MIX = 6,    // the fused scalar mix (ten rows, fifteen Variables: ScalarMixGD::row; eight / thirteen where v = 0)
                  // the small gadgets on Variables from elsewhere (scalar_gadgets.hpp) and the gate batches (composer.hpp): SegTemplate (permutation.hpp)
                  WIRES_SELECT_ZERO = 7, WIRES_SELECT_ONE = 8, WIRES_MAYBE_EQUAL = 9, WIRES_IS_NON_ZERO = 10, WIRES_GATE_OUT = 11,
                  WIRES_GATE_ROWS = 12, WIRES_KINDS = 13 };

// positions of an item that hold a witness allocated elsewhere, and the rank of (item-row j, wire w) among them in recording order:
// every item owns that many consecutive slots of the sparse list, so a lane knows where its entry goes without asking anybody
PG_FOOTPRINT_HD inline uint32_t ladder_foreign_per_item(uint32_t kind) {
    return kind == WIRES_RANGE_CHECK_ALLOCATED ? 4u : kind == WIRES_MAX_BOUND_ALLOCATED ? 2u : kind == WIRES_DECOMPOSITION ? 1u : 0u;
}
// positions of a full item that hold a Variable from elsewhere (= its slots on the sparse list; a short item leaves the rest as holes)
PG_FOOTPRINT_HD inline uint32_t template_foreign_per_item(uint32_t kind) {
    return kind == WIRES_SELECT_ZERO || kind == WIRES_MAYBE_EQUAL || kind == WIRES_IS_NON_ZERO || kind == WIRES_GATE_OUT ? 2u
           : kind == WIRES_SELECT_ONE || kind == WIRES_GATE_ROWS ? 3u : 0u;
}
PG_FOOTPRINT_HD inline bool is_template_kind(uint32_t kind) { return kind >= WIRES_MIX && kind < WIRES_KINDS; }

// ---- what an item of every kind weighs ------------------------------------------------------------------------------------------
// Rows and Variables of one item: a + b * n for the ladder kinds (n: the ladder length, PermSeg::wire_n), the full item's fixed
// figures for the template kinds (permutation.hpp asserts them against kSegTemplates).  A kind that allocates its own witness counts
// it: WIRES_RANGE_CHECK / WIRES_MAX_BOUND are their `_ALLOCATED` twins plus that one Variable (range.rs:82-113: 2n + 5 rows and
// n + 261 Variables per bound block, range_check two blocks and one row to join them).
struct KindShape {
    uint16_t rows, rows_per_bit, vars, vars_per_bit;
    uint8_t allocated_twin;  // the same gadget on a witness allocated earlier (0: the kind has no such twin)
};
constexpr KindShape kKindShapes[WIRES_KINDS] = {
    {0, 0, 0, 0, 0},                                    // WIRES_UNKNOWN
    {11, 4, 524, 2, WIRES_RANGE_CHECK_ALLOCATED},       // WIRES_RANGE_CHECK
    {5, 2, 262, 1, WIRES_MAX_BOUND_ALLOCATED},          // WIRES_MAX_BOUND
    {11, 4, 523, 2, 0},                                 // WIRES_RANGE_CHECK_ALLOCATED
    {5, 2, 261, 1, 0},                                  // WIRES_MAX_BOUND_ALLOCATED
    {4, 2, 260, 1, 0},                                  // WIRES_DECOMPOSITION
    {10, 0, 15, 0, 0},                                  // WIRES_MIX
    {1, 0, 1, 0, 0},                                    // WIRES_SELECT_ZERO
    {4, 0, 4, 0, 0},                                    // WIRES_SELECT_ONE
    {3, 0, 3, 0, 0},                                    // WIRES_MAYBE_EQUAL
    {3, 0, 3, 0, 0},                                    // WIRES_IS_NON_ZERO
    {1, 0, 1, 0, 0},                                    // WIRES_GATE_OUT
    {1, 0, 0, 0, 0},                                    // WIRES_GATE_ROWS
};
constexpr uint32_t kind_rows(uint32_t kind, uint64_t n = 0) { return kKindShapes[kind].rows + kKindShapes[kind].rows_per_bit * (uint32_t)n; }
constexpr uint32_t kind_vars(uint32_t kind, uint64_t n = 0) { return kKindShapes[kind].vars + kKindShapes[kind].vars_per_bit * (uint32_t)n; }
// WIRES_RANGE_CHECK / WIRES_MAX_BOUND as called: `fused` with the allocate of its witness, or on a witness allocated earlier
constexpr uint32_t ladder_kind(uint32_t fused_kind, bool fused) { return fused ? fused_kind : kKindShapes[fused_kind].allocated_twin; }
// wire positions of an item that reference a Variable from elsewhere: its slots on the sparse list (what the sigma kernels use)
inline uint32_t kind_foreign(uint32_t kind) { return is_template_kind(kind) ? template_foreign_per_item(kind) : ladder_foreign_per_item(kind); }
// ... and what a call adds per item to pg_composer::sparse_hint, the first-pass size of that list: the same figure, except
// decomposition's 2 -- an estimate only (too large costs 8 bytes per item, too small a second pass); the kernels go by kind_foreign
inline uint32_t kind_sparse_hint(uint32_t kind) { return kind == WIRES_DECOMPOSITION ? 2u : kind_foreign(kind); }

// `items` items of one kind from (gate0, var0) on, every one creating all of its V Variables itself on its own L rows (and `tail` more,
// PermSeg::tail): a uniform footprint for the f-rows, which may then use closed forms instead of the gather and the sparse list
inline PermSeg footprint(uint64_t gate0, uint64_t var0, uint64_t items, uint32_t wire_kind, uint32_t wire_n = 0, uint32_t tail = 0) {
    const uint32_t L = kind_rows(wire_kind, wire_n) + tail, V = kind_vars(wire_kind, wire_n);
    return PermSeg{gate0, gate0 + items * L, var0, var0 + items * V, L, V, items, nullptr, nullptr, 1, wire_kind, wire_n, 0, tail, nullptr};
}

// a run of queued single calls, or a batch of rows-only gates, leaves a footprint from this many rows on; pg_composer_materialize
// leaves shorter ones to the generic gather (a footprint is a launch of its own in both f-rows)
constexpr uint32_t kFootprintMinRows = 4096;

// ---- pg_composer_permutation ------------------------------------------------------------------------------------------------------
constexpr uint32_t kPermLocalLdsLimit = 64 * 1024 - 256;
constexpr uint32_t kPermNone = 0xFFFF, kPermDone = 0xFFFE;
// perm_item_kernel's dynamic LDS for an item (or group) of L rows and V Variables (permutation.hpp)
PG_FOOTPRINT_HD inline uint32_t perm_local_lds_bytes(uint32_t L, uint32_t V) {
    return 4 * V + 2 * (V + 2) + 2 * (3 * L + 3 * L + L) + L + 16;
}
#ifndef PG_PERM_LADDER_ROWS
#define PG_PERM_LADDER_ROWS 512
#endif
#ifndef PG_PERM_LADDER_LDS
#define PG_PERM_LADDER_LDS 39936
#endif
#ifndef PG_PERM_LDS_PAD
#define PG_PERM_LDS_PAD 0
#endif
constexpr uint32_t kPermLadderRows = PG_PERM_LADDER_ROWS;  // rows per workgroup piece (a multiple of 2 * kThreads): permutation.hpp, perm_ladder_kernel
constexpr uint32_t kPermLadderLds = PG_PERM_LADDER_LDS;    // dynamic LDS per workgroup, unused: bounds how many are resident per CU

enum PermRoute : uint32_t {
    PERM_ITEMS = 0,        // perm_item_kernel: counting sort of the item's (group's) positions in LDS, the wires read back
    PERM_LADDER,           // perm_ladder_kernel<false>: a uniform ladder gadget's rows in closed form
    PERM_LADDER_RAGGED,    // perm_ladder_kernel<true>: max_bound with a bound per item
    PERM_TEMPLATE,         // perm_template_kernel<false>: the small gadgets, the fused mix, the gate batches -- from the kind's wire table
    PERM_TEMPLATE_RAGGED,  // perm_template_kernel<true>: the same with items that stopped at is_non_zero's error
};
// The questions are asked in this order (it decides where more than one could say yes; no footprint that is created does that:
// template kinds have wire_n == 0, and of the ladder kinds only WIRES_MAX_BOUND and WIRES_RANGE_CHECK are ever ragged -- a bound, or a
// (min, max) pair, per item -- never with a tail -- capi_composer.inc, add_footprint, asserts both.  Ragged WIRES_RANGE_CHECK has no closed
// form yet: it answers no question and falls to PERM_ITEMS, and to the windowed MAT_READ_WIRES below).
inline PermRoute perm_route(const PermSeg &s) {
    if (s.wire_kind != WIRES_UNKNOWN && !s.row_off && s.wire_n >= 2) return PERM_LADDER;
    if (is_template_kind(s.wire_kind) && s.tail == 0) return s.row_off ? PERM_TEMPLATE_RAGGED : PERM_TEMPLATE;
    if (s.row_off && s.wire_kind == WIRES_MAX_BOUND && s.tail == 0) return PERM_LADDER_RAGGED;
    return PERM_ITEMS;
}
// `k` consecutive items of the footprint fit one workgroup of perm_item_kernel
inline bool perm_fits(const PermSeg &s, uint64_t k) {
    return 4 * k * s.L < kPermDone && k * s.V < kPermNone && perm_local_lds_bytes((uint32_t)(k * s.L), (uint32_t)(k * s.V)) <= kPermLocalLdsLimit;
}
// PermSeg::group for the pass; 0: not even one item fits a workgroup's LDS -- the footprint is dropped, its rows count as rows of
// single calls.  Small items are linked several at a time (about 1024 rows per workgroup).  The closed-form routes put EVERY position
// that holds a Variable from elsewhere on the sparse list -- also one that holds a Variable of an earlier item of the same footprint
// (calls of one kind merge into one footprint: the second call's inputs may be the first one's results) -- so perm_splice_kernel must
// take an item's local positions from the item's OWN rows, not from a group's: group 1.
inline uint32_t perm_group(const PermSeg &s, PermRoute route) {
    if (!perm_fits(s, 1)) return 0;
    // (a template kind on the ladder route -- wire_n >= 2, which no footprint has -- with a tail: never forced, and not here either)
    if (route == PERM_LADDER ? !is_template_kind(s.wire_kind) || s.tail == 0 : route != PERM_ITEMS) return 1;
    uint64_t k = 1024 / s.L;
    k = k < 1 ? 1 : (k > s.items ? s.items : k);
    while (k > 1 && !perm_fits(s, k)) k--;
    return (uint32_t)k;
}
// the route's slots on the sparse list, handed out in closed form ahead of what the other kernels reserve by counter:
// whether the footprint gets a sparse_base at all, and how many slots per item
inline bool perm_reserves_slots(PermRoute route) { return route == PERM_LADDER || route == PERM_TEMPLATE || route == PERM_TEMPLATE_RAGGED; }
inline uint32_t perm_slots_per_item(const PermSeg &s, PermRoute route) {
    return route == PERM_LADDER ? ladder_foreign_per_item(s.wire_kind) : perm_reserves_slots(route) ? template_foreign_per_item(s.wire_kind) : 0u;
}
// the ragged closed forms find a row's item in a window of the call's prefix sums, from the first item of the row's piece
// (PermSeg::piece_item, perm_piece_items_kernel)
inline bool perm_needs_piece_items(PermRoute route) { return route == PERM_LADDER_RAGGED || route == PERM_TEMPLATE_RAGGED; }
// workgroup pieces of kPermLadderRows rows, counted from the even gate at or before the footprint's first (the closed-form routes)
inline uint64_t perm_pieces(const PermSeg &s) { return (s.gate_end - (s.gate_base & ~1ull) + kPermLadderRows - 1) / kPermLadderRows; }
// dynamic LDS of the route's launch.  The closed forms use none: the allocation bounds the workgroups resident per CU to four
// short-lived ones where nothing is read back; rows that reference a Variable from elsewhere read it back, those waves wait for
// memory and more of them resident hide it -- full residency (no allocation) for such footprints
inline uint32_t perm_lds_bytes(const PermSeg &s, PermRoute route) {
    switch (route) {
    case PERM_LADDER: return ladder_foreign_per_item(s.wire_kind) ? 0u : kPermLadderLds;
    case PERM_LADDER_RAGGED: return kPermLadderLds;
    case PERM_TEMPLATE:
    case PERM_TEMPLATE_RAGGED: return template_foreign_per_item(s.wire_kind) ? 0u : kPermLadderLds - 8192;
    default: return perm_local_lds_bytes(s.group * s.L, s.group * s.V) + PG_PERM_LDS_PAD;
    }
}

// ---- pg_composer_materialize ------------------------------------------------------------------------------------------------------
constexpr uint32_t kMatWindowVars = 1040;  // two windows of 33 280 B: two workgroups per CU (fewer, fatter store streams: -3 %); range_check's 1034 Variables per item fit
// how the store waves of materialize_items_kernel learn a row's three Variables
enum : int {
    MAT_READ_WIRES = 0,  // from the wire columns (any batched call)
    MAT_SELF = 2,        // in closed form (PermSeg::wire_kind = KIND, compiled in: one instantiation per kind keeps the wire functions
                         // of the others -- and their registers -- out), and the store waves load NOTHING: the rows that come along
                         // from the next group and the ONE Variable per item that may come from elsewhere (the witness of the
                         // `_allocated` kinds and of scalar_decomposition) get their values from the loader; such groups have at most
                         // kMatWitItems items
};
constexpr uint32_t kMatWitItems = 4;  // (these kinds create >= 257 Variables per item: a window holds at most four)
constexpr uint32_t kMatMixRaggedItems = 127;  // the ragged fused mix: fewer than that many items per group (materialize.hpp, kOff = 128 prefix sums)

// consecutive items whose Variables fit one LDS window: a workgroup's share
inline uint64_t mat_group(const PermSeg &s) {
    const uint64_t group = kMatWindowVars / (s.V ? s.V : 1);
    return group < 1 ? 1 : (group > s.items ? s.items : group);
}
// materialize_items_kernel<mode, kind, ragged>, or -- windowed false -- the footprint is left to the generic gather of the gap it widens
// (items that outgrow the window or create nothing, calls too small to bother)
struct MatRoute {
    bool windowed;
    int mode;
    uint32_t kind;
    bool ragged;
};
inline MatRoute mat_route(const PermSeg &s, uint64_t group) {
    if (s.V > kMatWindowVars || s.V == 0 || s.gate_end - s.gate_base < kFootprintMinRows) return MatRoute{false, MAT_READ_WIRES, WIRES_UNKNOWN, false};
    if (s.row_off) {
        // per-item bounds: closed form from the prefix sums; the fused mix with items that stopped at their error: two shapes
        if (s.wire_kind == WIRES_MAX_BOUND && group <= kMatWitItems) return MatRoute{true, MAT_SELF, WIRES_MAX_BOUND, true};
        if (s.wire_kind == WIRES_MIX && group < kMatMixRaggedItems) return MatRoute{true, MAT_SELF, WIRES_MIX, true};
        return MatRoute{true, MAT_READ_WIRES, WIRES_UNKNOWN, false};
    }
    // the wires in closed form (not even the indices are read), at most one Variable per item from elsewhere -- and then at most
    // kMatWitItems items per group; the kinds from WIRES_MIX on keep MAT_READ_WIRES (their wires are data)
    if (s.wire_kind != WIRES_UNKNOWN && s.wire_kind <= WIRES_MIX && (ladder_foreign_per_item(s.wire_kind) == 0 || group <= kMatWitItems))
        return MatRoute{true, MAT_SELF, s.wire_kind, false};
    return MatRoute{true, MAT_READ_WIRES, WIRES_UNKNOWN, false};
}

}  // namespace pg
