// tests/cpp/digest_host.cpp -- the host build of csrc/digest.hpp (g++, also under -fsanitize=address,undefined), for
// tests/test_digest_host.py: what the digest of an append's device arrays promises, on fixed seeded arrays of 1, 2, 63, 64, 65 and
// 1000 words.
//   * PARTITION: the digest does not depend on which lane adds which word nor on the order of summation -- the words dealt to 1, 64 and
//     256 strided lanes, each lane and then the lanes summed forwards and backwards, against one loop over the array;
//   * DISTINCTION: it changes (at least one of its two words) when one entry changes, when two entries of one array change places,
//     when two arrays of one call change places, when two items' bounds change places (the pairs digested as interval_bounds_kernel
//     does: eight words an item), and when an entry moves between two arrays of a call;
//   * SALTS: the named salts are pairwise different.
// Prints "ok <checks>" and returns 0, or says what failed (the first 20, each line starting with its group) and returns 1.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "digest.hpp"

using namespace pg;
typedef unsigned long long u64;

static int failures = 0, checks = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        checks++;                         \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
        }                                 \
    } while (0)

static std::vector<u64> seeded(size_t n, u64 seed) {  // splitmix64
    std::vector<u64> a(n);
    for (size_t i = 0; i < n; i++) {
        u64 z = (seed += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        a[i] = z ^ (z >> 31);
    }
    return a;
}
static bool same(const Digest &x, const Digest &y) { return x.h1 == y.h1 && x.h2 == y.h2; }
static void sum(Digest &into, const Digest &d) {
    into.h1 += d.h1;
    into.h2 += d.h2;
}

// one loop over the array, added to d
static void digest(Digest &d, const std::vector<u64> &a, u64 salt) {
    for (size_t i = 0; i < a.size(); i++) d.add(a[i], i, salt);
}
static Digest digest(const std::vector<u64> &a, u64 salt) {
    Digest d{0, 0};
    digest(d, a, salt);
    return d;
}
// the words dealt to `lanes` strided lanes as a kernel's grid does
static Digest dealt(const std::vector<u64> &a, u64 salt, size_t lanes, bool lane_backwards, bool lanes_backwards) {
    std::vector<Digest> part(lanes, Digest{0, 0});
    const size_t n = a.size();
    for (size_t l = 0; l < lanes; l++) {
        std::vector<size_t> mine;
        for (size_t i = l; i < n; i += lanes) mine.push_back(i);
        for (size_t k = 0; k < mine.size(); k++) {
            const size_t i = mine[lane_backwards ? mine.size() - 1 - k : k];
            part[l].add(a[i], i, salt);
        }
    }
    Digest d{0, 0};
    for (size_t l = 0; l < lanes; l++) sum(d, part[lanes_backwards ? lanes - 1 - l : l]);
    return d;
}
// the bounds of `items` items as interval_bounds_kernel digests them: lo and hi of four words an item, eight words an item in one array
static Digest bounds(const std::vector<u64> &lo, const std::vector<u64> &hi) {
    Digest d{0, 0};
    for (size_t i = 0; i < lo.size() / 4; i++)
        for (size_t j = 0; j < 8; j++) d.add(j < 4 ? lo[4 * i + j] : hi[4 * i + j - 4], 8 * i + j, scalar_array_salt(0));
    return d;
}

int main() {
    const size_t sizes[] = {1, 2, 63, 64, 65, 1000};
    for (size_t n : sizes) {
        const std::vector<u64> a = seeded(n, 1000 + n), b = seeded(n, 2000 + n);
        const u64 sa = var_array_salt(0), sb = var_array_salt(1);
        const Digest whole = digest(a, sa);
        // PARTITION
        for (size_t lanes : {(size_t)1, (size_t)64, (size_t)256})
            for (int order = 0; order < 4; order++)
                CHECK(same(dealt(a, sa, lanes, order & 1, order & 2), whole), "partition: %zu words over %zu lanes, order %d", n, lanes, order);
        // DISTINCTION
        {
            std::vector<u64> c = a;
            c[n / 2] += 1;
            CHECK(!same(digest(c, sa), whole), "distinction: %zu words, entry %zu changed", n, n / 2);
        }
        if (n >= 2) {
            std::vector<u64> c = a;
            std::swap(c[0], c[n - 1]);
            CHECK(!same(digest(c, sa), whole), "distinction: %zu words, entries 0 and %zu exchanged", n, n - 1);
            c = a;
            std::swap(c[n / 2 - 1], c[n / 2]);
            CHECK(!same(digest(c, sa), whole), "distinction: %zu words, entries %zu and %zu exchanged", n, n / 2 - 1, n / 2);
        }
        {
            Digest ab = whole, ba = digest(b, sa);
            digest(ab, b, sb);
            digest(ba, a, sb);
            CHECK(!same(ab, ba), "distinction: two arrays of %zu words exchanged", n);
            std::vector<u64> a2 = a, b2 = b;  // an entry of one array and the entry at its place in the other, exchanged
            std::swap(a2[n / 2], b2[n / 2]);
            Digest moved = digest(a2, sa);
            digest(moved, b2, sb);
            CHECK(!same(ab, moved), "distinction: entry %zu moved between two arrays of %zu words", n / 2, n);
            // ... and the weighted sum's: a coefficient and a constant
            Digest cs = digest(a, kSaltCoeff), cs2 = digest(a2, kSaltCoeff);
            digest(cs, b, kSaltConstant);
            digest(cs2, b2, kSaltConstant);
            CHECK(!same(cs, cs2), "distinction: entry %zu moved between coefficients and constants of %zu words", n / 2, n);
        }
        if (n >= 2) {  // n items' bounds
            std::vector<u64> lo = seeded(4 * n, 3000 + n), hi = seeded(4 * n, 4000 + n);
            const Digest was = bounds(lo, hi);
            for (size_t j = 0; j < 4; j++) {
                std::swap(lo[j], lo[4 * (n - 1) + j]);
                std::swap(hi[j], hi[4 * (n - 1) + j]);
            }
            CHECK(!same(bounds(lo, hi), was), "distinction: the bounds of items 0 and %zu of %zu exchanged", n - 1, n);
            CHECK(!same(bounds(hi, lo), bounds(lo, hi)), "distinction: the two bound arrays of %zu items exchanged", n);
        }
    }
    // SALTS
    const u64 salts[] = {var_array_salt(0), var_array_salt(1),    var_array_salt(2), scalar_array_salt(0),
                         scalar_array_salt(1), kSaltSegOff, kSaltCoeff,        kSaltConstant};
    const size_t n_salts = sizeof salts / sizeof salts[0];
    for (size_t i = 0; i < n_salts; i++)
        for (size_t j = i + 1; j < n_salts; j++) CHECK(salts[i] != salts[j], "salts: %zu and %zu are equal", i, j);
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("ok %d\n", checks);
    return 0;
}
