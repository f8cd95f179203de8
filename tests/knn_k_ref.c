/* tests/knn_k_ref.c -- TEST REFERENCE: brute-force k nearest points in fp32, the library's contract restated in plain C.
 * d = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with dx = q.x - m.x in float (compiled with -ffp-contract=off, so nothing else
 * fuses), the k smallest by (distance, row) ascending: rows are visited in ascending order and a row displaces a list entry
 * only when strictly nearer, so ties keep the lowest row.  Slots past M: idx -1, dist +inf.  A NaN distance never enters.
 * Points are column-major (x = p[i], y = p[i + ld], z = p[i + 2 ld]); idx / dist are [Q][k] row-major.  Threads split the
 * queries (at most 16). */
#include <math.h>
#include <pthread.h>
#include <stdint.h>

typedef struct {
    const float *q, *m;
    int Q, ldq, M, ldm, k, t, nt;
    int32_t* idx;
    float* dist;
} job_t;

static void* run(void* arg) {
    const job_t* j = (const job_t*)arg;
    for (int i = j->t; i < j->Q; i += j->nt) {
        float* d = j->dist + (size_t)i * j->k;
        int32_t* x = j->idx + (size_t)i * j->k;
        for (int s = 0; s < j->k; ++s) { d[s] = INFINITY; x[s] = -1; }
        const float qx = j->q[i], qy = j->q[i + (size_t)j->ldq], qz = j->q[i + 2 * (size_t)j->ldq];
        int n = 0;                                          /* filled slots */
        for (int r = 0; r < j->M; ++r) {
            const float dx = qx - j->m[r], dy = qy - j->m[r + (size_t)j->ldm], dz = qz - j->m[r + 2 * (size_t)j->ldm];
            const float v = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (v != v) continue;
            if (n == j->k && !(v < d[j->k - 1])) continue;
            int p = n < j->k ? n++ : j->k - 1;
            while (p > 0 && v < d[p - 1]) { d[p] = d[p - 1]; x[p] = x[p - 1]; --p; }
            d[p] = v; x[p] = r;
        }
    }
    return 0;
}

int knn_k_ref(const float* q, int Q, int ldq, const float* m, int M, int ldm, int k, int32_t* idx, float* dist, int threads) {
    if (k < 1 || Q < 0 || M < 0) return 1;
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    pthread_t th[16];
    job_t jobs[16];
    for (int t = 0; t < threads; ++t) {
        jobs[t] = (job_t){q, m, Q, ldq, M, ldm, k, t, threads, idx, dist};
        if (pthread_create(&th[t], 0, run, &jobs[t])) return 2;
    }
    for (int t = 0; t < threads; ++t) pthread_join(th[t], 0);
    return 0;
}
