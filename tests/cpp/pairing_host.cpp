// tests/cpp/pairing_host.cpp -- the host build of csrc/fq2.hpp, fq12.hpp, g2.hpp and pairing.hpp (the code the device runs,
// compiled by g++, also under -fsanitize=undefined,address): reads operations and Montgomery limbs from the file named on the
// command line, one per line, and prints each result's limbs, for tests/test_pairing_host.py to compare with
// tests/pairing_model.py limb for limb.
//   f2 <op> a b        op: add sub neg mul sqr inv conj xi dbl            -> 12 limbs
//   f12 <op> a b       op: add sub neg mul sqr inv conj frob frob2        -> 72 limbs
//   sparse f l0 l2 l3  f (l0 + l2 w^2 + l3 w^3)                            -> 72 limbs
//   prep q             the 68 lines of the ate loop over q                 -> 68 x 24 limbs
//   pair n (p q) x n   the conjugated Miller value, then its final power   -> 72 + 72 limbs
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pairing.hpp"
using namespace pg;

static FILE *in;
static uint64_t limb() {
    uint64_t v = 0;
    if (std::fscanf(in, "%" SCNx64, &v) != 1) std::exit(3);
    return v;
}
static Fq rd_fq() {
    Fq a;
    for (int i = 0; i < 6; i++) a.l[i] = limb();
    return a;
}
static Fq2 rd_f2() {
    Fq2 a;
    a.c0 = rd_fq();
    a.c1 = rd_fq();
    return a;
}
static Fq12 rd_f12() {
    Fq12 a;
    for (int k = 0; k < 6; k++) a.c[k] = rd_f2();
    return a;
}
static void pr(const Fq &a) {
    for (int i = 0; i < 6; i++) std::printf("%" PRIx64 " ", a.l[i]);
}
static void pr(const Fq2 &a) { pr(a.c0), pr(a.c1); }
static void pr(const Fq12 &a) {
    for (int k = 0; k < 6; k++) pr(a.c[k]);
}

int main(int argc, char **argv) {
    if (argc < 2 || !(in = std::fopen(argv[1], "r"))) return 2;
    char kind[16], op[16];
    while (std::fscanf(in, "%15s", kind) == 1) {
        const std::string k = kind;
        if (k == "f2") {
            if (std::fscanf(in, "%15s", op) != 1) return 3;
            const std::string o = op;
            const Fq2 a = rd_f2(), b = rd_f2();
            pr(o == "add" ? fq2_add(a, b) : o == "sub" ? fq2_sub(a, b) : o == "neg" ? fq2_neg(a) : o == "mul" ? fq2_mul(a, b)
               : o == "sqr" ? fq2_square(a) : o == "inv" ? fq2_inverse(a) : o == "conj" ? fq2_conj(a) : o == "xi" ? fq2_mul_xi(a)
                                                                                                                 : fq2_dbl(a));
        } else if (k == "f12") {
            if (std::fscanf(in, "%15s", op) != 1) return 3;
            const std::string o = op;
            const Fq12 a = rd_f12(), b = rd_f12();
            pr(o == "add" ? fq12_add(a, b) : o == "sub" ? fq12_sub(a, b) : o == "neg" ? fq12_neg(a) : o == "mul" ? fq12_mul(a, b)
               : o == "sqr" ? fq12_square(a) : o == "inv" ? fq12_invert(a) : o == "conj" ? fq12_conj(a)
               : o == "frob" ? fq12_frobenius(a) : fq12_frobenius2(a));
        } else if (k == "sparse") {
            const Fq12 f = rd_f12();
            const Fq2 l0 = rd_f2(), l2 = rd_f2();
            const Fq l3 = rd_fq();
            pr(fq12_mul_sparse(f, l0, l2, l3));
        } else if (k == "prep") {
            G2A q;
            q.x = rd_f2();
            q.y = rd_f2();
            std::vector<G2Line> lines(kAteLines);
            g2_prepare(q, lines.data());
            for (const G2Line &ln : lines) pr(ln.c0), pr(ln.c2);
        } else if (k == "pair") {
            const int n = (int)limb();
            std::vector<G1A> ps(n);
            std::vector<std::vector<G2Line>> lines(n, std::vector<G2Line>(kAteLines));
            std::vector<const G2Line *> lp(n);
            for (int j = 0; j < n; j++) {
                ps[j].x = rd_fq();
                ps[j].y = rd_fq();
                G2A q;
                q.x = rd_f2();
                q.y = rd_f2();
                g2_prepare(q, lines[j].data());
                lp[j] = lines[j].data();
            }
            const Fq12 f = pairing_host_miller(ps.data(), lp.data(), n);
            pr(f);
            pr(pairing_host_final_exp(f));
        } else {
            return 4;
        }
        std::printf("\n");
    }
    return 0;
}
