// tests/cpp/g1_host.cpp -- the host build of csrc/g1.hpp's group law (the code the device runs, compiled by g++, also under
// -fsanitize=undefined,address) one operation at a time, for tests/test_g1_ops_host.py to compare with tests/g1_model.py.
//   g1_host <op> <n> <a> <b> <k> <out>
// a, b, k and out name files of raw little-endian limbs ("-": not used by the operation): n rows of G1X (24 limbs) or G1A (12
// limbs) as the operation says, k one uint32 per row; out receives n G1X rows, G1A rows for NEG_AFFINE.  The operations and
// their numbers are those of tests/cpp/g1_device_ops.hip.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "g1.hpp"
using namespace pg;

enum Op { ADD = 0, ADD_AFFINE, DBL, DBL_AFFINE, MUL_SMALL, FROM_AFFINE, NEG_AFFINE };

template <class T>
static std::vector<T> rd(const char *path, size_t n) {
    std::vector<T> v(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) std::exit(3);
    std::fclose(f);
    return v;
}

template <class T>
static void wr(const char *path, const std::vector<T> &v) {
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size() || std::fclose(f) != 0) std::exit(3);
}

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    const int op = std::atoi(argv[1]);
    const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
    const char *pa = argv[3], *pb = argv[4], *pk = argv[5], *po = argv[6];
    static_assert(sizeof(G1X) == 192 && sizeof(G1A) == 96, "rows are bare limbs");
    std::vector<G1X> out(n);
    if (op == ADD) {
        const auto a = rd<G1X>(pa, n), b = rd<G1X>(pb, n);
        for (size_t i = 0; i < n; i++) out[i] = g1x_add(a[i], b[i]);
    } else if (op == ADD_AFFINE) {
        const auto a = rd<G1X>(pa, n);
        const auto b = rd<G1A>(pb, n);
        for (size_t i = 0; i < n; i++) out[i] = g1x_add_affine(a[i], b[i]);
    } else if (op == DBL) {
        const auto a = rd<G1X>(pa, n);
        for (size_t i = 0; i < n; i++) out[i] = g1x_dbl(a[i]);
    } else if (op == DBL_AFFINE) {
        const auto a = rd<G1A>(pa, n);
        for (size_t i = 0; i < n; i++) out[i] = g1x_dbl_affine(a[i]);
    } else if (op == MUL_SMALL) {
        const auto a = rd<G1X>(pa, n);
        const auto k = rd<uint32_t>(pk, n);
        for (size_t i = 0; i < n; i++) out[i] = g1x_mul_small(a[i], k[i]);
    } else if (op == FROM_AFFINE) {
        const auto a = rd<G1A>(pa, n);
        for (size_t i = 0; i < n; i++) out[i] = g1x_from_affine(a[i]);
    } else if (op == NEG_AFFINE) {
        const auto a = rd<G1A>(pa, n);
        std::vector<G1A> neg(n);
        for (size_t i = 0; i < n; i++) neg[i] = g1a_neg(a[i]);
        wr(po, neg);
        return 0;
    } else {
        return 4;
    }
    wr(po, out);
    return 0;
}
