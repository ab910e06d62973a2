// tests/cpp/codec_host.cpp -- the host build of csrc/g1_codec.hpp (the code the device runs, compiled by g++, also under
// -fsanitize=undefined,address): reads operations from the file named on the command line, one per line, and prints each
// result, for tests/test_g1_codec_host.py to compare with tests/g1_codec_model.py.
//   dec <check> <96 hex digits>   g1_decode                -> status and the point's 12 limbs
//   chk <12 limbs>                g1a_check                -> status
//   enc <12 limbs>                g1_encode                -> 96 hex digits
//   mulu <12 limbs>               |u| P, made affine       -> 12 limbs
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "g1_codec.hpp"
using namespace pg;

static FILE *in;
static uint64_t limb() {
    uint64_t v = 0;
    if (std::fscanf(in, "%" SCNx64, &v) != 1) std::exit(3);
    return v;
}
static G1A rd_point() {
    G1A p;
    for (int i = 0; i < 6; i++) p.x.l[i] = limb();
    for (int i = 0; i < 6; i++) p.y.l[i] = limb();
    return p;
}
static void pr(const G1A &p) {
    for (int i = 0; i < 6; i++) std::printf("%" PRIx64 " ", p.x.l[i]);
    for (int i = 0; i < 6; i++) std::printf("%" PRIx64 " ", p.y.l[i]);
}

int main(int argc, char **argv) {
    if (argc < 2 || !(in = std::fopen(argv[1], "r"))) return 2;
    char kind[16];
    while (std::fscanf(in, "%15s", kind) == 1) {
        const std::string k = kind;
        if (k == "dec") {
            const uint64_t check = limb();
            char hex[128];
            if (std::fscanf(in, "%127s", hex) != 1 || std::strlen(hex) != 96) return 3;
            uint8_t bytes[48];
            for (int i = 0; i < 48; i++) {
                unsigned v = 0;
                if (std::sscanf(hex + 2 * i, "%2x", &v) != 1) return 3;
                bytes[i] = (uint8_t)v;
            }
            G1Bytes b;
            std::memcpy(b.w, bytes, 48);
            G1A p;
            const uint8_t st = g1_decode(b, check != 0, &p);
            std::printf("%x ", st);
            pr(p);
        } else if (k == "chk") {
            std::printf("%x", g1a_check(rd_point()));
        } else if (k == "enc") {
            const G1Bytes b = g1_encode(rd_point());
            uint8_t bytes[48];
            std::memcpy(bytes, b.w, 48);
            for (int i = 0; i < 48; i++) std::printf("%02x", bytes[i]);
        } else if (k == "mulu") {
            const G1X q = g1x_mul_u(g1x_from_affine(rd_point()));
            if (g1x_is_identity(q)) {
                pr(g1a_identity());
            } else {
                const Fq d = fq_invert(fq_mul(q.zz, q.zzz));  // 1 / (ZZ ZZZ): 1 / ZZ = d ZZZ, 1 / ZZZ = d ZZ
                const Fq izz = fq_mul(d, q.zzz), izzz = fq_mul(d, q.zz);
                pr(G1A{fq_mul(q.x, izz), fq_mul(q.y, izzz)});
            }
        } else {
            return 4;
        }
        std::printf("\n");
    }
    return 0;
}
