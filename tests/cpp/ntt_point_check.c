/* TEST INFRASTRUCTURE: the random-point identity of a forward NTT, on the host, for columns too large for Python integers
 * (tests/test_gpu_ntt.py builds it with oracle/fr.c as a second source).  e = fft(c) over the 2^m subgroup <omega> holds iff,
 * at a point s outside the subgroup (with overwhelming probability over s),
 *     sum_j e_j s^j == (s^n - 1) sum_i c_i / (omega^i s - 1)
 * All values are Montgomery limbs (fr_t).  Up to 16 threads, each over a contiguous range: Horner for the left side, Montgomery's
 * trick over batches of kBatch denominators (one inversion per batch) for the right side.
 * ntt_point_check_scaled is the same identity with c_i replaced by c_i g^i (each thread starts its power at g^lo): with e the
 * coset transform of c it covers all four kinds -- fft (c = in, e = out, g = 1), ifft (c = out, e = in, g = 1), coset_fft
 * (c = in, e = out, g) and coset_ifft (c = out, e = in, g). */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>

#include "fr.h"

#define kBatch 4096

typedef struct {
    const fr_t *c, *e;
    uint64_t lo, hi;
    fr_t s, omega, g;
    fr_t lhs, rhs; /* sum_{j in [lo, hi)} e_j s^j, sum_{i in [lo, hi)} c_i g^i / (omega^i s - 1) */
    int ok;
} part_t;

static fr_t pow_u64(fr_t b, uint64_t x) {
    const uint64_t by[4] = {x, 0, 0, 0};
    return fr_pow(b, by);
}

static void *run(void *arg) {
    part_t *p = (part_t *)arg;
    fr_t acc = FR_ZERO;
    for (uint64_t j = p->hi; j-- > p->lo;) acc = fr_add(fr_mul(acc, p->s), p->e[j]);
    p->lhs = fr_mul(acc, pow_u64(p->s, p->lo));
    fr_t *den = (fr_t *)malloc(3 * kBatch * sizeof(fr_t)), *pre = den + kBatch, *gp = pre + kBatch;
    if (!den) return NULL;
    fr_t x = fr_mul(pow_u64(p->omega, p->lo), p->s), gi = pow_u64(p->g, p->lo), sum = FR_ZERO, one = FR_ONE;
    const int scaled = !fr_eq(p->g, one); /* (g = 1, the plain transform: no products by g^i) */
    for (uint64_t b = p->lo; b < p->hi; b += kBatch) {
        const uint64_t cnt = p->hi - b < kBatch ? p->hi - b : kBatch;
        fr_t prod = one, inv;
        for (uint64_t k = 0; k < cnt; k++) {
            den[k] = fr_sub(x, one);
            pre[k] = prod;
            prod = fr_mul(prod, den[k]);
            x = fr_mul(x, p->omega);
            if (scaled) {
                gp[k] = gi;
                gi = fr_mul(gi, p->g);
            }
        }
        if (!fr_invert(prod, &inv)) {
            free(den);
            return NULL; /* s is in the subgroup: the caller picks another */
        }
        for (uint64_t k = cnt; k-- > 0;) {
            const fr_t ci = scaled ? fr_mul(p->c[b + k], gp[k]) : p->c[b + k];
            sum = fr_add(sum, fr_mul(ci, fr_mul(inv, pre[k])));
            inv = fr_mul(inv, den[k]);
        }
    }
    free(den);
    p->rhs = sum;
    p->ok = 1;
    return NULL;
}

/* 1: the identity holds, 0: it does not, -1: s is a root of unity of the subgroup or a thread failed */
int ntt_point_check_scaled(const uint64_t *c, const uint64_t *e, uint64_t n, const uint64_t s[4], const uint64_t omega[4],
                            const uint64_t g[4], int threads) {
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    part_t parts[16];
    pthread_t tid[16];
    fr_t fs, fo, fg;
    for (int i = 0; i < 4; i++) {
        fs.l[i] = s[i];
        fo.l[i] = omega[i];
        fg.l[i] = g[i];
    }
    for (int t = 0; t < threads; t++) {
        parts[t].c = (const fr_t *)c;
        parts[t].e = (const fr_t *)e;
        parts[t].lo = n * t / threads;
        parts[t].hi = n * (t + 1) / threads;
        parts[t].s = fs;
        parts[t].omega = fo;
        parts[t].g = fg;
        parts[t].ok = 0;
        if (pthread_create(&tid[t], NULL, run, &parts[t])) {
            for (int u = 0; u < t; u++) pthread_join(tid[u], NULL);
            return -1;
        }
    }
    fr_t lhs = FR_ZERO, rhs = FR_ZERO;
    int ok = 1;
    for (int t = 0; t < threads; t++) {
        pthread_join(tid[t], NULL);
        ok &= parts[t].ok;
        lhs = fr_add(lhs, parts[t].lhs);
        rhs = fr_add(rhs, parts[t].rhs);
    }
    if (!ok) return -1;
    const fr_t sn = fr_sub(pow_u64(fs, n), FR_ONE);
    return fr_eq(lhs, fr_mul(sn, rhs)) ? 1 : 0;
}

/* the identity of the plain transform: g = 1 */
int ntt_point_check(const uint64_t *c, const uint64_t *e, uint64_t n, const uint64_t s[4], const uint64_t omega[4], int threads) {
    const fr_t one = FR_ONE;
    return ntt_point_check_scaled(c, e, n, s, omega, one.l, threads);
}
