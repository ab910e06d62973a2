// tests/cpp/carve_host.cpp -- the host build of csrc/host_util.hpp's HIP-free part (pg::Carve; g++, also under
// -fsanitize=address,undefined), for tests/test_carve_host.py: runs every layout below through both passes and checks
//   * the measuring pass hands out no pointer at all;
//   * the placing pass hands out parts that start on a multiple of the alignment, in the order they were taken, each beginning
//     where the one before ended or later (a part of count 0 takes no room, so it starts where the next one does);
//   * the last part ends at or before the measured total, and every byte of every part can be written: the buffer is
//     allocated with exactly the measured size, so AddressSanitizer sees a part that runs past it;
//   * for pg_msm's and pg_poly_evaluate's workspaces the measured total is the closed form those calls used to allocate by.
// Prints "ok <layouts>" and returns 0, or says what failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_util.hpp"

struct B16 { unsigned char b[16]; };    // a uint4
struct B192 { unsigned char b[192]; };  // an extended Jacobian point of G1 (pg::G1X: four Fq)
struct B7 { unsigned char b[7]; };      // an odd size: every part of it needs padding

struct Part {
    const char *name;
    unsigned char *p;
    uint64_t bytes;
};

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            failures++;                   \
        }                                 \
    } while (0)

// a layout: the parts it names, in order; returns what Carve::bytes() says
typedef uint64_t (*Layout)(pg::Carve cv, std::vector<Part> &parts);

template <typename T>
static void part(pg::Carve &cv, std::vector<Part> &parts, const char *name, uint64_t count) {
    parts.push_back(Part{name, reinterpret_cast<unsigned char *>(cv.take<T>(count)), count * sizeof(T)});
}

// pg_msm (capi_msm.inc), n = 1000 scalars in n_cols = 2 columns, the sort asking for 12345 bytes
static const uint64_t kN = 1000, kCols = 2, kSortBytes = 12345;
static const uint64_t kRun = 64, kWindows = 16, kBuckets = 1u << 15, kSegs = 256;  // msm.hpp's kMsmRun, kMsmWindows, kMsmBuckets, kMsmSegs
static uint64_t msm_layout(pg::Carve cv, std::vector<Part> &parts) {
    const uint64_t lanes0 = (kN + kRun - 1) / kRun, partA = 2 * lanes0, partB = 2 * ((partA + kRun - 1) / kRun);
    part<uint64_t>(cv, parts, "k0", kN);
    part<uint64_t>(cv, parts, "k1", kN);
    part<char>(cv, parts, "sort_tmp", kSortBytes);
    part<uint32_t>(cv, parts, "pkA", partA);
    part<B192>(cv, parts, "ppA", partA);
    part<uint32_t>(cv, parts, "pkB", partB);
    part<B192>(cv, parts, "ppB", partB);
    part<B192>(cv, parts, "buckets", kWindows * (kBuckets + 1));
    part<B192>(cv, parts, "seg", kWindows * kSegs);
    part<B192>(cv, parts, "win", kWindows);
    part<B192>(cv, parts, "res", kCols);
    return cv.bytes();
}
static uint64_t r256(uint64_t b) { return (b + 255) / 256 * 256; }
static uint64_t msm_closed_form() {  // the eleven terms pg_msm summed before it allocated
    const uint64_t lanes0 = (kN + kRun - 1) / kRun, partA = 2 * lanes0, partB = 2 * ((partA + kRun - 1) / kRun);
    const uint64_t nbk = kWindows * (kBuckets + 1), nseg = kWindows * kSegs;
    return 2 * r256(kN * 8) + r256(kSortBytes) + r256(partA * 4) + r256(partA * 192) + r256(partB * 4) + r256(partB * 192) +
           r256(nbk * 192) + r256(nseg * 192) + r256(kWindows * 192) + r256(kCols * 192);
}

// pg_poly_evaluate (capi.hip), n_cols = 3 columns in segs = 2 segments: 16-byte units
static const uint64_t kEvalCols = 3, kEvalSegs = 2;
static uint64_t eval_layout(pg::Carve cv, std::vector<Part> &parts) {
    part<B16>(cv, parts, "lane", 2 * 256);
    part<B16>(cv, parts, "seg_lo", 2);
    part<B16>(cv, parts, "seg", 2 * kEvalSegs);
    part<B16>(cv, parts, "partial", 2 * kEvalCols * kEvalSegs);
    return cv.bytes();
}

// mixed element types, parts of count 0 at the start, in the middle and at the end
static uint64_t mixed_layout(pg::Carve cv, std::vector<Part> &parts) {
    part<uint64_t>(cv, parts, "empty first", 0);
    part<uint32_t>(cv, parts, "one word", 1);
    part<B7>(cv, parts, "sevens", 37);
    part<B192>(cv, parts, "empty middle", 0);
    part<char>(cv, parts, "one byte", 1);
    part<B16>(cv, parts, "units", 16);
    part<B192>(cv, parts, "points", 3);
    part<uint8_t>(cv, parts, "255 bytes", 255);
    part<uint8_t>(cv, parts, "257 bytes", 257);
    part<uint64_t>(cv, parts, "empty last", 0);
    return cv.bytes();
}
static uint64_t empty_layout(pg::Carve cv, std::vector<Part> &parts) {
    part<B16>(cv, parts, "nothing", 0);
    return cv.bytes();
}

static uint64_t run(const char *what, Layout layout, uint64_t align) {
    std::vector<Part> measured, placed;
    const uint64_t total = layout(pg::Carve(align), measured);
    for (const Part &m : measured) CHECK(m.p == nullptr, "%s/%llu: measuring handed out a pointer for %s", what, (unsigned long long)align, m.name);
    CHECK(total % align == 0, "%s/%llu: total %llu is no multiple of the alignment", what, (unsigned long long)align, (unsigned long long)total);
    // exactly `total` bytes (at least one, so that there is a base), aligned like a device allocation
    void *mem = nullptr;
    if (posix_memalign(&mem, 256, total ? total : 1)) std::exit(2);
    unsigned char *base = static_cast<unsigned char *>(mem);
    CHECK(layout(pg::Carve(align, base), placed) == total, "%s: the passes disagree about the total", what);
    CHECK(placed.size() == measured.size(), "%s: the passes disagree about the parts", what);
    uint64_t end = 0;  // of the parts so far, from the base
    for (const Part &q : placed) {
        const uint64_t at = (uint64_t)(q.p - base);
        CHECK(q.p != nullptr && at % align == 0, "%s/%llu: %s starts at %llu", what, (unsigned long long)align, q.name, (unsigned long long)at);
        CHECK(at >= end, "%s/%llu: %s starts at %llu, inside the part before (which ends at %llu)", what, (unsigned long long)align, q.name,
              (unsigned long long)at, (unsigned long long)end);
        if (q.bytes) CHECK(at == (end + align - 1) / align * align, "%s/%llu: %s leaves a hole", what, (unsigned long long)align, q.name);
        CHECK(at + q.bytes <= total, "%s/%llu: %s ends at %llu, past the total %llu", what, (unsigned long long)align, q.name,
              (unsigned long long)(at + q.bytes), (unsigned long long)total);
        if (at + q.bytes <= total) std::memset(q.p, 0xa5, q.bytes);
        if (q.bytes) end = at + q.bytes;
    }
    std::free(base);
    return total;
}

int main() {
    int layouts = 0;
    for (uint64_t align : {16, 256}) {
        run("mixed", mixed_layout, align);
        CHECK(run("empty", empty_layout, align) == 0, "an empty layout takes room");
        run("msm", msm_layout, align);
        run("eval", eval_layout, align);
        layouts += 4;
    }
    const uint64_t msm = run("msm", msm_layout, 256), eval = run("eval", eval_layout, 16);
    CHECK(msm == msm_closed_form(), "pg_msm's workspace: measured %llu, closed form %llu", (unsigned long long)msm,
          (unsigned long long)msm_closed_form());
    CHECK(eval == 32 * (257 + (kEvalCols + 1) * kEvalSegs), "pg_poly_evaluate's workspace: measured %llu, closed form %llu",
          (unsigned long long)eval, (unsigned long long)(32 * (257 + (kEvalCols + 1) * kEvalSegs)));
    // a worked case by hand, 256-byte alignment: 1 word -> 256; 37 x 7 = 259 bytes -> 512; 1 byte -> 256; 16 units -> 256;
    // 3 x 192 = 576 -> 768; 255 -> 256; 257 -> 512
    CHECK(run("mixed", mixed_layout, 256) == 256 + 512 + 256 + 256 + 768 + 256 + 512, "the mixed layout's total at 256");
    // and 16: 4 -> 16; 259 -> 272; 1 -> 16; 256; 576; 255 -> 256; 257 -> 272
    CHECK(run("mixed", mixed_layout, 16) == 16 + 272 + 16 + 256 + 576 + 256 + 272, "the mixed layout's total at 16");
    if (failures) return 1;
    std::printf("ok %d\n", layouts);
    return 0;
}
