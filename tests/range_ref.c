/* tests/range_ref.c -- TEST REFERENCE: brute-force radius search in fp32, the library's contract restated in plain C.
 * d = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with dx = q.x - m.x in float (compiled with -ffp-contract=off, so nothing else
 * fuses); row r belongs to query i iff d <= r2 as a float comparison (inclusive; NaN never passes; +inf <= +inf does).  Two
 * passes, as the library has: range_ref_count gives counts [Q]; the caller forms seg_off [Q + 1] (exclusive running sums);
 * range_ref_fill writes query i's rows at seg_off[i] .. seg_off[i + 1], sorted by (distance, row) ascending: d is never
 * negative or NaN inside a result, so (bits(d) << 32) | row sorts as an unsigned 64-bit key.
 * Points are column-major (x = p[i], y = p[i + ld], z = p[i + 2 ld]).  Threads split the queries (at most 16). */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    const float *q, *m;
    int Q, ldq, M, ldm, t, nt, err;
    float r2;
    int32_t* counts;
    const int64_t* seg_off;
    int32_t* idx;
    float* dist;
} job_t;

static float dist2(const job_t* j, float qx, float qy, float qz, int r) {
    const float dx = qx - j->m[r], dy = qy - j->m[r + (size_t)j->ldm], dz = qz - j->m[r + 2 * (size_t)j->ldm];
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
static int cmp_u64(const void* a, const void* b) {
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : x > y;
}

static void* run(void* arg) {
    job_t* j = (job_t*)arg;
    for (int i = j->t; i < j->Q; i += j->nt) {
        const float qx = j->q[i], qy = j->q[i + (size_t)j->ldq], qz = j->q[i + 2 * (size_t)j->ldq];
        if (!j->seg_off) {                                   /* pass 1 */
            int32_t n = 0;
            for (int r = 0; r < j->M; ++r) n += dist2(j, qx, qy, qz, r) <= j->r2;
            j->counts[i] = n;
            continue;
        }
        const int64_t b = j->seg_off[i], n = j->seg_off[i + 1] - b;
        if (n <= 0) continue;
        uint64_t* key = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)n);
        if (!key) { j->err = 3; return 0; }
        int64_t k = 0;
        for (int r = 0; r < j->M; ++r) {
            const float v = dist2(j, qx, qy, qz, r);
            if (v <= j->r2) {
                if (k == n) { j->err = 4; break; }           /* seg_off does not belong to these inputs */
                uint32_t bits;
                memcpy(&bits, &v, 4);
                key[k++] = ((uint64_t)bits << 32) | (uint32_t)r;
            }
        }
        if (k != n) j->err = 4;
        qsort(key, (size_t)k, sizeof(uint64_t), cmp_u64);
        for (int64_t s = 0; s < k; ++s) {
            const uint32_t bits = (uint32_t)(key[s] >> 32);
            memcpy(&j->dist[b + s], &bits, 4);
            j->idx[b + s] = (int32_t)(uint32_t)key[s];
        }
        free(key);
    }
    return 0;
}

static int launch(job_t base, int threads) {
    if (base.Q < 0 || base.M < 0) return 1;
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    pthread_t th[16];
    job_t jobs[16];
    for (int t = 0; t < threads; ++t) {
        jobs[t] = base; jobs[t].t = t; jobs[t].nt = threads; jobs[t].err = 0;
        if (pthread_create(&th[t], 0, run, &jobs[t])) return 2;
    }
    int err = 0;
    for (int t = 0; t < threads; ++t) { pthread_join(th[t], 0); if (jobs[t].err) err = jobs[t].err; }
    return err;
}

int range_ref_count(const float* q, int Q, int ldq, const float* m, int M, int ldm, float r2, int32_t* counts, int threads) {
    job_t b = {q, m, Q, ldq, M, ldm, 0, 1, 0, r2, counts, 0, 0, 0};
    return launch(b, threads);
}
int range_ref_fill(const float* q, int Q, int ldq, const float* m, int M, int ldm, float r2, const int64_t* seg_off, int32_t* idx,
                   float* dist, int threads) {
    job_t b = {q, m, Q, ldq, M, ldm, 0, 1, 0, r2, 0, seg_off, idx, dist};
    return launch(b, threads);
}
