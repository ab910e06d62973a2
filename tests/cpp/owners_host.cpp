// tests/cpp/owners_host.cpp -- the host build of csrc/owners.hpp over tests/cpp/stub/hip/hip_runtime.h (g++, also under
// -fsanitize=address,undefined), for tests/test_owners_host.py.  The stand-in runtime counts what is alive and refuses the k-th
// creation on request; this program checks
//   * Scratch and Pinned: grow, a refused grow leaves them empty, move construction / move assignment / self-move leave one owner;
//   * Event, Stream, Staging, CallBuffers: a refused creation is an error and leaves nothing behind; a Staging that was sent
//     waits for its event exactly once before it is refilled, one that was not does not wait;
//   * ColumnStore in both layouts: for EVERY k from the first to the last allocation of a create and of each kind of grow,
//     refusing allocation k is an error after which the store's view is byte for byte what it was, its capacities and contents
//     too, as many objects are alive as before and no error is left behind for hipGetLastError; the same for a copy that fails;
//     the allocation counts (nine separate arrays, one block, one array when only the Variables grow); what a successful grow copies;
//   * nothing is alive after any scope, nor at the end (and LeakSanitizer finds what the counts would miss).
// Prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstring>
#include <string>

#include "owners.hpp"

static int failures = 0, checks = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        checks++;                         \
        if (!(cond)) {                    \
            std::printf("line %d: ", __LINE__); \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            failures++;                   \
        }                                 \
    } while (0)

// the library's arithmetic is tested where the library is (tests/test_capi_exports.py): here any layout of disjoint parts will do
extern "C" pg_status pg_columns_slab_layout(uint64_t n_gates, uint64_t n_vars, uint64_t stride_bytes, uint64_t offsets[9],
                                            uint64_t *total_bytes) {
    const uint64_t sel = pg::round256(n_gates * 32), stride = stride_bytes > sel ? pg::round256(stride_bytes) : sel;
    for (int i = 0; i < 5; i++) offsets[i] = i * stride;
    uint64_t at = 4 * stride + sel;
    for (int i = 5; i < 8; i++, at += pg::round256(n_gates * 8)) offsets[i] = at;
    offsets[8] = at;
    *total_bytes = at + pg::round256(n_vars * 32);
    return PG_OK;
}

// refuse creation number k (counted from now) for the length of a scope
struct Refuse {
    explicit Refuse(long k) { g_hip.refuse = g_hip.created + k; }
    ~Refuse() { g_hip.refuse = -1; }
};

template <class Buf>
static void buffers(const char *what, const long &alive) {
    {
        Buf a;
        CHECK(a.reserve(100) == PG_OK && a.get() && a.size() == 100 && alive == 1, "%s: first reserve", what);
        std::memset(a.get(), 0x5a, 100);
        void *was = a.get();
        CHECK(a.reserve(50) == PG_OK && a.get() == was && a.size() == 100, "%s: a smaller reserve moves nothing", what);
        CHECK(a.reserve(1000) == PG_OK && a.size() == 1000 && alive == 1, "%s: growing leaves one allocation", what);
        std::memset(a.get(), 0x5a, 1000);
        {
            Refuse r(0);
            CHECK(a.reserve(5000) == PG_ERR_HIP && !a.get() && a.size() == 0 && alive == 0, "%s: a refused grow leaves it empty", what);
            CHECK(g_last_error.find("out of memory") != std::string::npos, "%s: the message names the runtime's error: %s", what, g_last_error.c_str());
        }
        (void)hipGetLastError();
        CHECK(a.reserve(64) == PG_OK && alive == 1, "%s: and it can be used again", what);
        was = a.get();
        Buf b(std::move(a));
        CHECK(!a.get() && a.size() == 0 && b.get() == was && b.size() == 64 && alive == 1, "%s: move construction", what);
        Buf c;
        CHECK(c.reserve(32) == PG_OK && alive == 2, "%s: a second buffer", what);
        c = std::move(b);
        CHECK(!b.get() && b.size() == 0 && c.get() == was && c.size() == 64 && alive == 1, "%s: move assignment releases what was there", what);
        Buf &same = c;
        c = std::move(same);
        CHECK(c.get() == was && c.size() == 64 && alive == 1, "%s: self-move", what);
        c = Buf();
        CHECK(!c.get() && alive == 0, "%s: assigning an empty one releases", what);
        CHECK(c.reserve(0) == PG_OK && !c.get() && alive == 0, "%s: nothing to reserve", what);
        CHECK(c.reserve(16) == PG_OK && alive == 1, "%s: left to the destructor", what);
    }
    CHECK(alive == 0 && g_hip.alive() == 0, "%s: alive after the scope", what);
}

static void carving() {
    Scratch s;
    uint64_t *a = nullptr;
    char *b = nullptr;
    const auto layout = [&](Carve cv) {
        a = cv.take<uint64_t>(3);
        b = cv.take<char>(7);
        return cv.bytes();
    };
    CHECK(s.carve(256, layout) == PG_OK && s.size() == 512 && (void *)a == s.get() && b == s.as<char>() + 256, "carve places its parts");
    std::memset(a, 1, 24);
    std::memset(b, 2, 7);
}

static void events_and_streams() {
    {
        Event e;
        Stream s, t;
        CHECK(e.create(hipEventDisableTiming) == PG_OK && e.get() && g_hip.events == 1, "event");
        CHECK(e.create(hipEventDisableTiming) == PG_OK && g_hip.events == 1, "an event is made once");
        CHECK(s.create(hipStreamNonBlocking) == PG_OK && s.get() && s.get()->priority == 0, "stream");
        CHECK(t.create_with_priority(hipStreamNonBlocking, -1) == PG_OK && t.get()->priority == -1 && g_hip.streams == 2, "stream with a priority");
        Event f;
        Stream u;
        Refuse r(0);
        CHECK(f.create(hipEventDisableTiming) == PG_ERR_HIP && !f.get() && g_hip.events == 1, "a refused event");
        g_hip.refuse = g_hip.created;
        CHECK(u.create(hipStreamNonBlocking) == PG_ERR_HIP && !u.get() && g_hip.streams == 2, "a refused stream");
    }
    (void)hipGetLastError();
    CHECK(g_hip.alive() == 0, "events and streams alive after the scope");
}

static void staging() {
    {
        Staging s;
        const long waits = g_hip.event_waits;
        CHECK(s.acquire(100, true) == PG_OK && s.size() == 100 && s.host() && s.device() && g_hip.alive() == 3, "staging pair");
        CHECK(s.acquire(0, true) == PG_OK && g_hip.event_waits == waits, "a pair that was never sent is refilled without a wait");
        std::memset(s.host(), 7, 100);
        CHECK(s.sent(nullptr) == hipSuccess, "sent");
        CHECK(s.acquire(0, true) == PG_OK && g_hip.event_waits == waits + 1, "a refill waits for the event of the copy that read it");
        CHECK(s.acquire(0, true) == PG_OK && g_hip.event_waits == waits + 1, "once");
        CHECK(s.sent(nullptr) == hipSuccess && s.acquire(400, true) == PG_OK && g_hip.event_waits == waits + 2 && s.size() == 400 && g_hip.alive() == 3,
              "growing waits too, and leaves one pair");
        CHECK(s.sent(nullptr) == hipSuccess && s.wait() == PG_OK && s.wait() == PG_OK && g_hip.event_waits == waits + 3, "wait()");
        {
            Refuse r(1);  // the pinned half grows, the twin is refused
            CHECK(s.acquire(1000, true) == PG_ERR_HIP && s.size() == 0 && !s.device(), "a refused twin leaves the pair at size 0");
        }
        (void)hipGetLastError();
        CHECK(s.acquire(1000, true) == PG_OK && s.size() == 1000 && s.device() && g_hip.alive() == 3, "and the next acquire allocates it again");
        Staging alone;  // the engine's use: no twin
        CHECK(alone.acquire(64, false) == PG_OK && alone.host() && !alone.device() && g_hip.device == 1 && g_hip.pinned == 2, "staging without a twin");
        Staging none;
        Refuse r(0);
        CHECK(none.acquire(8, true) == PG_ERR_HIP && g_hip.events == 2, "a refused event");
    }
    (void)hipGetLastError();
    CHECK(g_hip.alive() == 0, "staging alive after the scope");
}

static pg_status three_buffers(long refuse) {
    CallBuffers B(nullptr);
    uint64_t *a, *b;
    char *c;
    Refuse r(refuse);
    PG_TRY(B.take(&a, 80));
    PG_TRY(B.take(&b, 8));
    PG_TRY(B.take(&c, 3));
    std::memset(a, 1, 80);
    std::memset(b, 1, 8);
    std::memset(c, 1, 3);
    return g_hip.device == 3 ? PG_OK : PG_ERR_INVALID_ARGUMENT;
}
static void call_buffers() {
    CHECK(three_buffers(-1000) == PG_OK && g_hip.alive() == 0, "a call's buffers go with the call");
    for (long k = 0; k < 3; k++) CHECK(three_buffers(k) == PG_ERR_HIP && g_hip.alive() == 0, "a call that fails at buffer %ld leaves nothing", k);
    (void)hipGetLastError();
}

// ---- the column store -------------------------------------------------------------------------------------------------------
static void *column(const pg::ComposerCols &v, int i) { return i < 5 ? (void *)v.q[i] : i < 8 ? (void *)v.w[i - 5] : (void *)v.vars; }
static uint64_t unit(int i) { return i < 5 ? 32 : i < 8 ? 8 : 32; }
static unsigned char pattern(int i, uint64_t at) { return (unsigned char)(0x11 * (i + 1) + 3 * at); }
static void fill(const ColumnStore &s, uint64_t rows, uint64_t vars) {
    for (int i = 0; i < 9; i++) {
        unsigned char *p = static_cast<unsigned char *>(column(s.view(), i));
        for (uint64_t at = 0; at < (i < 8 ? rows : vars) * unit(i); at++) p[at] = pattern(i, at);
    }
}
static bool holds(const ColumnStore &s, uint64_t rows, uint64_t vars) {
    for (int i = 0; i < 9; i++) {
        const unsigned char *p = static_cast<const unsigned char *>(column(s.view(), i));
        if (!p) return false;
        for (uint64_t at = 0; at < (i < 8 ? rows : vars) * unit(i); at++)
            if (p[at] != pattern(i, at)) return false;
    }
    return true;
}
// every byte of every column up to the capacities can be written (ASan sees a column that is too short)
static void touch(const ColumnStore &s, uint64_t live_rows, uint64_t live_vars) {
    for (int i = 0; i < 9; i++) {
        const uint64_t live = (i < 8 ? live_rows : live_vars) * unit(i), cap = (i < 8 ? s.gate_cap() : s.var_cap()) * unit(i);
        std::memset(static_cast<unsigned char *>(column(s.view(), i)) + live, 0xee, cap - live);
    }
}
struct Snapshot {
    pg::ComposerCols view;
    uint64_t gate_cap, var_cap, stride;
    long alive;
    explicit Snapshot(const ColumnStore &s) : view(s.view()), gate_cap(s.gate_cap()), var_cap(s.var_cap()), stride(s.stride()), alive(g_hip.alive()) {}
    bool same(const ColumnStore &s) const {
        return std::memcmp(&view, &s.view(), sizeof view) == 0 && gate_cap == s.gate_cap() && var_cap == s.var_cap() && stride == s.stride() &&
               alive == g_hip.alive();
    }
};

static const uint64_t kRows = 5, kVars = 7;  // live in every store below

// `s` grows to (gate_cap, var_cap, stride), which takes `allocations` allocations and `copies` copies: first with each of them
// failing in turn, then for good
static void grow_checked(const char *what, ColumnStore &s, uint64_t gate_cap, uint64_t var_cap, uint64_t stride, long allocations, long copies,
                         long alive_after) {
    const Snapshot before(s);
    for (long k = 0; k < allocations; k++) {
        Refuse r(k);
        const long created = g_hip.created;
        const pg_status st = s.grow(gate_cap, var_cap, stride, kRows, kVars, nullptr);
        CHECK(st == PG_ERR_CAPACITY && g_last_error.find("composer cannot grow to " + std::to_string(gate_cap) + " rows / ") == 0,
              "%s, allocation %ld refused: status %d, %s", what, k, (int)st, g_last_error.c_str());
        CHECK(g_hip.created == created + k + 1, "%s, allocation %ld refused: %ld allocations tried", what, k, g_hip.created - created);
        CHECK(before.same(s), "%s, allocation %ld refused: the store changed, or %ld objects are alive instead of %ld", what, k, g_hip.alive(), before.alive);
        CHECK(holds(s, kRows, kVars), "%s, allocation %ld refused: the contents changed", what, k);
        CHECK(hipGetLastError() == hipSuccess, "%s, allocation %ld refused: the error is left behind", what, k);
    }
    for (long k = 0; k < copies; k++) {
        g_hip.refuse_copy = g_hip.copies + k;
        const pg_status st = s.grow(gate_cap, var_cap, stride, kRows, kVars, nullptr);
        g_hip.refuse_copy = -1;
        CHECK(st == PG_ERR_HIP && g_last_error.find("growing the composer: ") == 0, "%s, copy %ld failed: status %d, %s", what, k, (int)st, g_last_error.c_str());
        CHECK(before.same(s) && holds(s, kRows, kVars), "%s, copy %ld failed: the store changed", what, k);
        (void)hipGetLastError();
    }
    const long created = g_hip.created, copied = g_hip.copies;
    CHECK(s.grow(gate_cap, var_cap, stride, kRows, kVars, nullptr) == PG_OK, "%s: %s", what, g_last_error.c_str());
    CHECK(g_hip.created == created + allocations && g_hip.copies == copied + copies, "%s: %ld allocations and %ld copies, not %ld and %ld", what,
          g_hip.created - created, g_hip.copies - copied, allocations, copies);
    CHECK(s.gate_cap() == (gate_cap > before.gate_cap ? gate_cap : before.gate_cap) && s.var_cap() == (var_cap > before.var_cap ? var_cap : before.var_cap) &&
              s.stride() == stride, "%s: capacities %llu / %llu", what, (unsigned long long)s.gate_cap(), (unsigned long long)s.var_cap());
    CHECK(g_hip.alive() == alive_after, "%s: %ld objects alive, not %ld", what, g_hip.alive(), alive_after);
    CHECK(holds(s, kRows, kVars), "%s: the live part was not copied", what);
    touch(s, kRows, kVars);
}

static void column_store() {
    {
        for (long k = 0; k < 9; k++) {
            ColumnStore s;
            Refuse r(k);
            const pg::ComposerCols none{};
            CHECK(s.create(8, 8) == PG_ERR_CAPACITY && std::memcmp(&s.view(), &none, sizeof none) == 0 && s.gate_cap() == 0 && g_hip.alive() == 0,
                  "create, allocation %ld refused", k);
            CHECK(hipGetLastError() == hipSuccess, "create, allocation %ld refused: the error is left behind", k);
        }
        ColumnStore s;
        const long created = g_hip.created;
        CHECK(s.create(8, 8) == PG_OK && g_hip.created == created + 9 && g_hip.device == 9 && s.gate_cap() == 8 && s.var_cap() == 8 && s.stride() == 0,
              "create: nine allocations");
        fill(s, kRows, kVars);
        touch(s, kRows, kVars);
        const Snapshot made(s);
        CHECK(s.grow(8, 8, 0, kRows, kVars, nullptr) == PG_OK && s.grow(3, 2, 0, kRows, kVars, nullptr) == PG_OK && made.same(s) && g_hip.created == created + 9,
              "a grow that asks for no more does nothing");
        // separate arrays: only what grows moves
        const pg::ComposerCols v0 = s.view();
        grow_checked("separate, variables only", s, 8, 20, 0, 1, 1, 9);
        CHECK(std::memcmp(v0.q, s.view().q, sizeof v0.q) == 0 && std::memcmp(v0.w, s.view().w, sizeof v0.w) == 0 && v0.vars != s.view().vars,
              "only the Variables' array moves");
        const pg::ComposerCols v1 = s.view();
        grow_checked("separate, rows only", s, 16, 20, 0, 8, 8, 9);
        CHECK(v1.vars == s.view().vars && v1.q[0] != s.view().q[0] && v1.w[2] != s.view().w[2], "only the row arrays move");
        grow_checked("separate, both", s, 33, 41, 0, 9, 9, 9);
        // into one block, the block grows, and back
        grow_checked("into a block", s, 33, 41, 4096, 1, 9, 1);
        const unsigned char *q0 = reinterpret_cast<const unsigned char *>(s.view().q[0]);
        CHECK(reinterpret_cast<const unsigned char *>(s.view().q[1]) == q0 + 4096 && reinterpret_cast<const unsigned char *>(s.view().vars) > q0 + 4 * 4096,
              "the block's selector columns lie a stride apart");
        grow_checked("a block grows", s, 40, 41, 4096, 1, 9, 1);
        grow_checked("another stride", s, 40, 41, 8192, 1, 9, 1);
        {
            const Snapshot before(s);
            g_hip.free_bytes = 1000;
            const pg_status st = s.grow(64, 64, 8192, kRows, kVars, nullptr);
            g_hip.free_bytes = ~(size_t)0;
            CHECK(st == PG_ERR_CAPACITY && g_last_error.find("must exist beside the old one") != std::string::npos && before.same(s) && holds(s, kRows, kVars),
                  "a block that does not fit beside the old one: %s", g_last_error.c_str());
        }
        grow_checked("back to separate arrays", s, 40, 41, 0, 9, 9, 9);
    }
    CHECK(g_hip.alive() == 0, "columns alive after the scope");
}

int main() {
    buffers<Scratch>("Scratch", g_hip.device);
    buffers<Pinned>("Pinned", g_hip.pinned);
    carving();
    events_and_streams();
    staging();
    call_buffers();
    column_store();
    CHECK(g_hip.device == 0 && g_hip.pinned == 0 && g_hip.events == 0 && g_hip.streams == 0, "alive at the end: %ld device, %ld pinned, %ld events, %ld streams",
          g_hip.device, g_hip.pinned, g_hip.events, g_hip.streams);
    if (failures) return 1;
    std::printf("ok %d\n", checks);
    return 0;
}
