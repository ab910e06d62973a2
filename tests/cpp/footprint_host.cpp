// tests/cpp/footprint_host.cpp -- the host build of csrc/footprint.hpp (g++, also under -fsanitize=address,undefined), for
// tests/test_footprint_host.py: which kernel pg_composer_permutation and pg_composer_materialize give a footprint, and what an item
// of every kind weighs.
//   * SWEEP: every combination of kind, uniform / ragged, tail, ladder length and a list of shapes that sit on, just below and just
//     above every threshold; at each point perm_route / perm_group / the reserved slots / the pieces / the LDS size and mat_group /
//     mat_route must equal what the predicates did that pg_composer_permutation and pg_composer_materialize spelled out, several times
//     over, before footprint.hpp was written (old_perm, old_mat below: copied from there, condition by condition, in their order);
//   * TABLE: the routes of the footprints that real calls leave, one line per public batch entry point and per form of a flushed run,
//     written by hand -- what is meant to happen, readable without running anything;
//   * SHAPES: kind_rows / kind_vars against the closed forms of pg_range_check_layout, pg_max_bound_layout and
//     pg_scalar_decomposition_layout as they were spelled before they read the table.
// Prints "ok <sweep points> <table lines>" and returns 0, or says what failed (the first 20) and returns 1.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "footprint.hpp"

using namespace pg;

static int failures = 0;
#define CHECK(cond, ...)                                \
    do {                                                \
        if (!(cond)) {                                  \
            if (failures++ < 20) {                      \
                std::printf(__VA_ARGS__);               \
                std::printf("\n");                      \
            }                                           \
        }                                               \
    } while (0)

// ---- what the parent of footprint.hpp did --------------------------------------------------------------------------------------
enum OldKernel { OLD_ITEM, OLD_LADDER, OLD_LADDER_RAGGED, OLD_TEMPLATE, OLD_TEMPLATE_RAGGED };
struct OldPerm {
    bool kept;
    uint32_t group;
    bool has_base;
    uint64_t slots;
    bool needs_pieces;
    OldKernel kernel;
    uint64_t pieces;
    uint32_t lds;
};
static OldPerm old_perm(PermSeg s) {
    OldPerm o{};
    // the loop that kept the segments one workgroup can link in LDS and chose `group`
    const auto fits = [&](uint64_t k) {
        return 4 * k * s.L < kPermDone && k * s.V < kPermNone && perm_local_lds_bytes((uint32_t)(k * s.L), (uint32_t)(k * s.V)) <= kPermLocalLdsLimit;
    };
    if (!fits(1)) return o;
    o.kept = true;
    uint64_t k = 1024 / s.L;
    k = k < 1 ? 1 : (k > s.items ? s.items : k);
    while (k > 1 && !fits(k)) k--;
    const bool closed_ladder = s.wire_kind != WIRES_UNKNOWN && s.wire_kind < WIRES_MIX && (s.row_off ? s.wire_kind == WIRES_MAX_BOUND && s.tail == 0 : s.wire_n >= 2);
    if (closed_ladder || (is_template_kind(s.wire_kind) && s.tail == 0)) k = 1;
    s.group = o.group = (uint32_t)k;
    // the loop that reserved slots on the sparse list
    if (s.wire_kind != WIRES_UNKNOWN && !s.row_off && s.wire_n >= 2) {
        o.has_base = true;
        o.slots = s.items * ladder_foreign_per_item(s.wire_kind);
    } else if (is_template_kind(s.wire_kind) && s.tail == 0) {
        o.has_base = true;
        o.slots = s.items * template_foreign_per_item(s.wire_kind);
    }
    // the lambdas
    const auto ragged_ladder = [](const PermSeg &s) { return s.row_off && s.wire_kind == WIRES_MAX_BOUND && s.tail == 0; };
    const auto template_seg = [](const PermSeg &s) { return is_template_kind(s.wire_kind) && s.tail == 0; };
    const auto needs_pieces = [&](const PermSeg &s) { return ragged_ladder(s) || (template_seg(s) && s.row_off); };
    const auto pieces_of = [](const PermSeg &s) { return (s.gate_end - (s.gate_base & ~1ull) + kPermLadderRows - 1) / kPermLadderRows; };
    o.needs_pieces = needs_pieces(s);
    // the launch loop
    if (s.wire_kind != WIRES_UNKNOWN && !s.row_off && s.wire_n >= 2) {
        o.pieces = (s.gate_end - (s.gate_base & ~1ull) + kPermLadderRows - 1) / kPermLadderRows;
        o.lds = ladder_foreign_per_item(s.wire_kind) ? 0u : kPermLadderLds;
        o.kernel = OLD_LADDER;
        return o;
    }
    if (template_seg(s)) {
        o.pieces = pieces_of(s);
        o.lds = template_foreign_per_item(s.wire_kind) ? 0u : kPermLadderLds - 8192;
        o.kernel = s.row_off ? OLD_TEMPLATE_RAGGED : OLD_TEMPLATE;
        return o;
    }
    if (ragged_ladder(s)) {
        o.pieces = pieces_of(s);
        o.lds = kPermLadderLds;
        o.kernel = OLD_LADDER_RAGGED;
        return o;
    }
    o.lds = perm_local_lds_bytes(s.group * s.L, s.group * s.V) + PG_PERM_LDS_PAD;
    o.kernel = OLD_ITEM;
    return o;
}

struct OldMat {
    bool windowed;
    uint64_t group;
    int mode;
    uint32_t kind;
    bool ragged;
};
static OldMat old_mat(const PermSeg &s) {
    if (s.V > kMatWindowVars || s.V == 0 || s.gate_end - s.gate_base < 4096) return OldMat{false, 0, 0, 0, false};
    uint64_t group = kMatWindowVars / (s.V ? s.V : 1);
    group = group < 1 ? 1 : (group > s.items ? s.items : group);
    const bool closed = s.wire_kind != WIRES_UNKNOWN && !s.row_off && (ladder_foreign_per_item(s.wire_kind) == 0 || group <= kMatWitItems);
    if (s.row_off && s.wire_kind == WIRES_MAX_BOUND && group <= kMatWitItems) return OldMat{true, group, MAT_SELF, WIRES_MAX_BOUND, true};
    else if (s.row_off && s.wire_kind == WIRES_MIX && group < 127) return OldMat{true, group, MAT_SELF, WIRES_MIX, true};
    else if (!closed) return OldMat{true, group, MAT_READ_WIRES, WIRES_UNKNOWN, false};
    else if (s.wire_kind == WIRES_RANGE_CHECK) return OldMat{true, group, MAT_SELF, WIRES_RANGE_CHECK, false};
    else if (s.wire_kind == WIRES_MAX_BOUND) return OldMat{true, group, MAT_SELF, WIRES_MAX_BOUND, false};
    else if (s.wire_kind == WIRES_RANGE_CHECK_ALLOCATED) return OldMat{true, group, MAT_SELF, WIRES_RANGE_CHECK_ALLOCATED, false};
    else if (s.wire_kind == WIRES_MAX_BOUND_ALLOCATED) return OldMat{true, group, MAT_SELF, WIRES_MAX_BOUND_ALLOCATED, false};
    else if (s.wire_kind == WIRES_DECOMPOSITION) return OldMat{true, group, MAT_SELF, WIRES_DECOMPOSITION, false};
    else if (s.wire_kind == WIRES_MIX) return OldMat{true, group, MAT_SELF, WIRES_MIX, false};
    else return OldMat{true, group, MAT_READ_WIRES, WIRES_UNKNOWN, false};
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------------
static OldKernel as_old(PermRoute r) {
    switch (r) {
    case PERM_LADDER: return OLD_LADDER;
    case PERM_LADDER_RAGGED: return OLD_LADDER_RAGGED;
    case PERM_TEMPLATE: return OLD_TEMPLATE;
    case PERM_TEMPLATE_RAGGED: return OLD_TEMPLATE_RAGGED;
    default: return OLD_ITEM;
    }
}
static void point(const PermSeg &in) {
    char where[160];
    std::snprintf(where, sizeof where, "kind %u %s tail %u n %u L %u V %u items %llu gate_base %llu", in.wire_kind, in.row_off ? "ragged" : "uniform",
                  in.tail, in.wire_n, in.L, in.V, (unsigned long long)in.items, (unsigned long long)in.gate_base);
    const OldPerm o = old_perm(in);
    PermSeg s = in;
    const PermRoute route = perm_route(s);
    s.group = perm_group(s, route);
    CHECK((s.group != 0) == o.kept, "sweep: %s: kept %d, was %d", where, s.group != 0, o.kept);
    if (o.kept && s.group) {
        CHECK(as_old(route) == o.kernel, "sweep: %s: route %d, the launch loop took %d", where, (int)as_old(route), (int)o.kernel);
        CHECK(s.group == o.group, "sweep: %s: group %u, was %u", where, s.group, o.group);
        CHECK(perm_reserves_slots(route) == o.has_base, "sweep: %s: sparse_base set %d, was %d", where, perm_reserves_slots(route), o.has_base);
        CHECK(s.items * perm_slots_per_item(s, route) == o.slots, "sweep: %s: %llu reserved slots, were %llu", where,
              (unsigned long long)(s.items * perm_slots_per_item(s, route)), (unsigned long long)o.slots);
        CHECK(perm_needs_piece_items(route) == o.needs_pieces, "sweep: %s: piece_item %d, was %d", where, perm_needs_piece_items(route), o.needs_pieces);
        if (o.kernel != OLD_ITEM) CHECK(perm_pieces(s) == o.pieces, "sweep: %s: %llu pieces, were %llu", where, (unsigned long long)perm_pieces(s), (unsigned long long)o.pieces);
        CHECK(perm_lds_bytes(s, route) == o.lds, "sweep: %s: %u bytes of LDS, were %u", where, perm_lds_bytes(s, route), o.lds);
    }
    const OldMat m = old_mat(in);
    const uint64_t group = mat_group(in);
    const MatRoute r = mat_route(in, group);
    CHECK(r.windowed == m.windowed, "sweep: %s: materialize windowed %d, was %d", where, r.windowed, m.windowed);
    if (r.windowed && m.windowed)
        CHECK(group == m.group && r.mode == m.mode && r.kind == m.kind && r.ragged == m.ragged,
              "sweep: %s: materialize <%d, %u, %d> group %llu, was <%d, %u, %d> group %llu", where, r.mode, r.kind, r.ragged, (unsigned long long)group, m.mode,
              m.kind, m.ragged, (unsigned long long)m.group);
}

// (L, V, items): on, below and above every threshold
static const struct { uint32_t L, V; uint64_t items; } kShapes[] = {
    {1, 1, 4095}, {1, 1, 4096}, {1, 1, 4097},          // the 4096 rows from which materialize takes a footprint
    {3, 3, 1365}, {3, 3, 1366},                        // ... is_non_zero's items: 4095 and 4098 rows
    {10, 15, 409}, {10, 15, 410},                      // ... the fused mix: 4090 and 4100
    {43, 540, 95}, {43, 540, 96},                      // ... range_check at n = 8: 4085 and 4128
    {515, 517, 7}, {515, 517, 8},                      // ... max_bound at n = 255: 3605 and 4120
    {1, 0, 5000},                                      // rows-only gates: no Variable
    {5, 1039, 1000}, {5, 1040, 1000}, {5, 1041, 1000},  // kMatWindowVars
    {5, 261, 1000}, {5, 260, 1000}, {5, 208, 1000}, {5, 207, 1000},  // groups of 3, 4, 5, 5: kMatWitItems
    {1100, 100, 4}, {900, 100, 5},                     // ... groups of 4 and 5 because that is all the items there are
    {40, 8, 126}, {40, 8, 127}, {40, 8, 128},          // the ragged mix's 127 items per group
    {4350, 0, 2}, {4351, 0, 2}, {4351, 1, 2},          // the largest item perm_item_kernel's LDS holds, and the first that it does not
    {16384, 1, 1},                                     // ... nor its 16-bit positions
    {1, 15, 5000}, {9, 15, 1000}, {1024, 1, 10}, {1025, 1, 10}, {4, 4, 2000},  // groups of about 1024 rows, shrunk until they fit
};
static const uint64_t kDummyOffsets[2] = {0, 0};  // (never read: a ragged footprint is one whose row_off is not null)

static uint64_t sweep() {
    uint64_t points = 0;
    for (uint32_t kind = 0; kind < WIRES_KINDS; kind++)
        for (int ragged = 0; ragged < 2; ragged++)
            for (uint32_t tail : {0u, 1u, 8u})
                for (uint32_t n : {0u, 1u, 2u, 8u, 255u})
                    for (const auto &sh : kShapes)
                        for (uint64_t gate_base : {1000ull, 1001ull}) {
                            PermSeg s{gate_base, gate_base + sh.items * sh.L, 77, 77 + sh.items * sh.V, sh.L, sh.V, sh.items, nullptr, nullptr, 1, kind, n, 0, tail, nullptr};
                            if (ragged) s.row_off = s.var_off = kDummyOffsets;
                            point(s);
                            points++;
                        }
    return points;
}

// ---- the footprints of real calls ------------------------------------------------------------------------------------------------
static PermSeg ragged(PermSeg f) {
    f.row_off = f.var_off = kDummyOffsets;
    f.wire_n = 0;
    return f;
}
static const MatRoute kGather{false, MAT_READ_WIRES, WIRES_UNKNOWN, false}, kReadWires{true, MAT_READ_WIRES, WIRES_UNKNOWN, false};
static MatRoute self(uint32_t kind, bool is_ragged = false) { return MatRoute{true, MAT_SELF, kind, is_ragged}; }
static int table() {
    const uint64_t B = 10000;  // items: every footprint here has more than 4096 rows
    const struct {
        const char *call;
        PermSeg f;
        PermRoute sigma;
        MatRoute mat;
    } lines[] = {
        {"pg_composer_range_check_batch", footprint(3, 5, B, WIRES_RANGE_CHECK, 8), PERM_LADDER, self(WIRES_RANGE_CHECK)},
        {"pg_composer_range_check_allocated_batch", footprint(3, 5, B, WIRES_RANGE_CHECK_ALLOCATED, 8), PERM_LADDER, self(WIRES_RANGE_CHECK_ALLOCATED)},
        {"pg_composer_max_bound_batch", footprint(3, 5, B, WIRES_MAX_BOUND, 64), PERM_LADDER, self(WIRES_MAX_BOUND)},
        {"pg_composer_max_bound_allocated_batch", footprint(3, 5, B, WIRES_MAX_BOUND_ALLOCATED, 64), PERM_LADDER, self(WIRES_MAX_BOUND_ALLOCATED)},
        {"pg_composer_scalar_decomposition_batch", footprint(3, 5, B, WIRES_DECOMPOSITION, 255), PERM_LADDER, self(WIRES_DECOMPOSITION)},
        {"pg_composer_scalar_decomposition_batch, one bit", footprint(3, 5, B, WIRES_DECOMPOSITION, 1), PERM_ITEMS, self(WIRES_DECOMPOSITION)},
        {"pg_composer_max_bound_ragged_batch", ragged(footprint(3, 5, B, WIRES_MAX_BOUND, 255)), PERM_LADDER_RAGGED, self(WIRES_MAX_BOUND, true)},
        {"pg_composer_is_non_zero_batch", footprint(3, 5, B, WIRES_IS_NON_ZERO), PERM_TEMPLATE, kReadWires},
        {"pg_composer_is_non_zero_batch, failing items", ragged(footprint(3, 5, B, WIRES_IS_NON_ZERO)), PERM_TEMPLATE_RAGGED, kReadWires},
        {"pg_composer_scalar_mix_batch", footprint(3, 5, B, WIRES_MIX), PERM_TEMPLATE, self(WIRES_MIX)},
        {"pg_composer_scalar_mix_batch, failing items", ragged(footprint(3, 5, B, WIRES_MIX)), PERM_TEMPLATE_RAGGED, self(WIRES_MIX, true)},
        {"pg_composer_conditionally_select_zero_batch", footprint(3, 5, B, WIRES_SELECT_ZERO), PERM_TEMPLATE, kReadWires},
        {"pg_composer_conditionally_select_one_batch", footprint(3, 5, B, WIRES_SELECT_ONE), PERM_TEMPLATE, kReadWires},
        {"pg_composer_maybe_equal_batch", footprint(3, 5, B, WIRES_MAYBE_EQUAL), PERM_TEMPLATE, kReadWires},
        {"pg_composer_add_batch / pg_composer_mul_batch", footprint(3, 5, B, WIRES_GATE_OUT), PERM_TEMPLATE, kReadWires},
        {"pg_composer_poly_gate_batch / _constrain_to_constant_batch / _boolean_gate_batch", footprint(3, 5, B, WIRES_GATE_ROWS), PERM_TEMPLATE, kGather},
        // runs of queued single calls (flush): allocate + gadget, the gadget on a witness allocated earlier, and either with `tail`
        // rows-only gates on the result behind every call
        {"a run of allocate + range_check", footprint(3, 5, B, ladder_kind(WIRES_RANGE_CHECK, true), 8), PERM_LADDER, self(WIRES_RANGE_CHECK)},
        {"a run of range_check", footprint(3, 5, B, ladder_kind(WIRES_RANGE_CHECK, false), 8), PERM_LADDER, self(WIRES_RANGE_CHECK_ALLOCATED)},
        {"a run of allocate + max_bound", footprint(3, 5, B, ladder_kind(WIRES_MAX_BOUND, true), 8), PERM_LADDER, self(WIRES_MAX_BOUND)},
        {"a run of max_bound", footprint(3, 5, B, ladder_kind(WIRES_MAX_BOUND, false), 8), PERM_LADDER, self(WIRES_MAX_BOUND_ALLOCATED)},
        {"a loop of allocate + range_check + constrain_to_constant", footprint(3, 5, B, WIRES_RANGE_CHECK, 8, 1), PERM_LADDER, self(WIRES_RANGE_CHECK)},
        {"a loop of max_bound + two gates on its result", footprint(3, 5, B, WIRES_MAX_BOUND_ALLOCATED, 8, 2), PERM_LADDER, self(WIRES_MAX_BOUND_ALLOCATED)},
    };
    int n = 0;
    for (const auto &l : lines) {
        PermSeg s = l.f;
        const PermRoute route = perm_route(s);
        const MatRoute r = mat_route(s, mat_group(s));
        CHECK(route == l.sigma, "table: %s: sigma route %d, meant %d", l.call, (int)route, (int)l.sigma);
        CHECK(route == PERM_ITEMS ? perm_group(s, route) > 1 : perm_group(s, route) == 1, "table: %s: group %u", l.call, perm_group(s, route));
        CHECK(r.windowed == l.mat.windowed && r.mode == l.mat.mode && r.kind == l.mat.kind && r.ragged == l.mat.ragged,
              "table: %s: materialize <%d, %u, %d> windowed %d", l.call, r.mode, r.kind, r.ragged, r.windowed);
        n++;
    }
    return n;
}

// ---- rows and Variables per item -----------------------------------------------------------------------------------------------
static void shapes() {
    for (uint64_t n : {1ull, 2ull, 64ull, 255ull}) {
        // pg_range_check_layout: gates_per_item = 4n + 11, vars_per_item = 2n + 524 (2n + 523 of range_check + 1 of allocate)
        CHECK(kind_rows(WIRES_RANGE_CHECK, n) == 4 * n + 11 && kind_vars(WIRES_RANGE_CHECK, n) == 2 * n + 524, "shapes: range_check at n = %llu", (unsigned long long)n);
        CHECK(kind_rows(WIRES_RANGE_CHECK_ALLOCATED, n) == 4 * n + 11 && kind_vars(WIRES_RANGE_CHECK_ALLOCATED, n) == 2 * n + 523, "shapes: range_check_allocated at n = %llu", (unsigned long long)n);
        // pg_max_bound_layout: 2n + 5, n + 262 (n + 261 of max_bound + 1 of allocate)
        CHECK(kind_rows(WIRES_MAX_BOUND, n) == 2 * n + 5 && kind_vars(WIRES_MAX_BOUND, n) == n + 262, "shapes: max_bound at n = %llu", (unsigned long long)n);
        CHECK(kind_rows(WIRES_MAX_BOUND_ALLOCATED, n) == 2 * n + 5 && kind_vars(WIRES_MAX_BOUND_ALLOCATED, n) == n + 261, "shapes: max_bound_allocated at n = %llu", (unsigned long long)n);
        // pg_scalar_decomposition_layout: 2 num_bits + 4, num_bits + 260
        CHECK(kind_rows(WIRES_DECOMPOSITION, n) == 2 * n + 4 && kind_vars(WIRES_DECOMPOSITION, n) == n + 260, "shapes: decomposition at n = %llu", (unsigned long long)n);
    }
    CHECK(ladder_kind(WIRES_RANGE_CHECK, true) == WIRES_RANGE_CHECK && ladder_kind(WIRES_RANGE_CHECK, false) == WIRES_RANGE_CHECK_ALLOCATED &&
              ladder_kind(WIRES_MAX_BOUND, true) == WIRES_MAX_BOUND && ladder_kind(WIRES_MAX_BOUND, false) == WIRES_MAX_BOUND_ALLOCATED,
          "shapes: the fused / allocated pairing");
    // what the calls said they reference from elsewhere, per item (their literals): the kernels' figure, and decomposition's estimate
    const uint32_t hints[WIRES_KINDS] = {0, 0, 0, 4, 2, 2, 0, 2, 3, 2, 2, 2, 3};
    for (uint32_t k = 0; k < WIRES_KINDS; k++) {
        CHECK(kind_sparse_hint(k) == hints[k], "shapes: kind %u adds %u per item to sparse_hint", k, kind_sparse_hint(k));
        CHECK(kind_foreign(k) == (k == WIRES_DECOMPOSITION ? 1u : hints[k]), "shapes: kind %u has %u foreign positions", k, kind_foreign(k));
    }
}

int main() {
    const uint64_t points = sweep();
    const int lines = table();
    shapes();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("ok %llu %d\n", (unsigned long long)points, lines);
    return 0;
}
