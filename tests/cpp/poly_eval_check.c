/* TEST INFRASTRUCTURE: sum_{i < n} c_i x^i on the host, for columns too large for Python integers (tests/test_gpu_poly_evaluate.py
 * builds it with oracle/fr.c as a second source).  All values are Montgomery limbs (fr_t).  Up to 16 threads, each running Horner
 * over a contiguous range [lo, hi) and multiplying its sum by x^lo. */
#include <pthread.h>
#include <stdint.h>

#include "fr.h"

typedef struct {
    const fr_t *c;
    uint64_t lo, hi;
    fr_t x, sum;
} part_t;

static void *run(void *arg) {
    part_t *p = (part_t *)arg;
    fr_t acc = FR_ZERO;
    for (uint64_t i = p->hi; i-- > p->lo;) acc = fr_add(fr_mul(acc, p->x), p->c[i]);
    const uint64_t by[4] = {p->lo, 0, 0, 0};
    p->sum = fr_mul(acc, fr_pow(p->x, by));
    return NULL;
}

/* out = sum_i c_i x^i; 0 on success, -1 if a thread could not be started */
int poly_eval_check(const uint64_t *c, uint64_t n, const uint64_t x[4], int threads, uint64_t out[4]) {
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    part_t parts[16];
    pthread_t tid[16];
    fr_t fx;
    for (int i = 0; i < 4; i++) fx.l[i] = x[i];
    int started = 0, rc = 0;
    for (int t = 0; t < threads; t++) {
        parts[t].c = (const fr_t *)c;
        parts[t].lo = n * t / threads;
        parts[t].hi = n * (t + 1) / threads;
        parts[t].x = fx;
        if (pthread_create(&tid[t], NULL, run, &parts[t])) {
            rc = -1;
            break;
        }
        started++;
    }
    fr_t sum = FR_ZERO;
    for (int t = 0; t < started; t++) {
        pthread_join(tid[t], NULL);
        sum = fr_add(sum, parts[t].sum);
    }
    for (int i = 0; i < 4; i++) out[i] = sum.l[i];
    return rc;
}
