// pcreg_amd/csrc/unique_rows.hip -- [C, ia] = unique(A, 'rows') for n x 3 doubles on the device, and the aggregation of putative
// matches built on it (completeExperiment.m:439-443).  DESIGN 4.12.
//
// Order.  Every double is mapped to a u64 whose unsigned order is the numeric order: negative values have all bits flipped, the
// others the sign bit; -0 is mapped as +0 (for the key only: C = A(ia,:) is read from A and keeps its bits).  -inf < finite < +inf
// as numbers.  A NaN is ordered by its mapped bit pattern (positive NaNs above +inf, negative ones below -inf, two NaNs equal iff
// their bits are): not MATLAB's rule -- the host tier refuses NaN rows, the device tier documents this.  Any input terminates and
// stays in bounds: nothing below depends on the values being ordered consistently with anything but the u64 compare.
//
// Record.  The FULL record travels: three keys and the original row, 28 bytes, as four arrays (k0 | k1 | k2 | row) so that every
// access of a wave is contiguous.  (The alternative, a permutation with the keys re-read through it, makes every compare of every
// merge pass a gather of three doubles n rows apart.)  The total order is (k0, k1, k2, row): no two records compare equal, so the
// result is a pure function of the input, equal rows lie in ascending row order and the head of a run is its smallest row --
// MATLAB's default 'first'.
//
//   U1  unique_tile_sort_kernel   T = 2048 rows per workgroup: keys formed from A, a bitonic network over the four LDS arrays
//                                 (56 KB, inside the 64 KB a kernel has without the large-LDS attribute), sorted records out
//   U2  unique_merge_kernel       ceil(log2(n_cap / T)) passes over ping-pong buffers, one launch each: runs of L records are
//                                 merged pairwise; a workgroup owns output records [2048 c, 2048 c + 2048) of its pair, finds the two
//                                 merge-path splits that bound them by binary search (threads 0 and 1), stages the <= 2048 input
//                                 records in LDS and places every one by its rank: own position + lower bound in the other side
//   U3  unique_count_kernel       heads (record 0, or any key differs from the record before) per chunk of 2048 records
//   U4  unique_compact_kernel     every chunk adds the counts of the chunks before it, scans its own heads, writes ia; the chunk
//                                 that holds record n - 1 writes n_unique (chunk 0 when n = 0)
// No kernel waits for another workgroup; every loop is a binary search over registers or a fixed trip count.  n is read from
// device memory by every kernel (clamped into [0, n_cap]); the grid and the number of passes follow n_cap alone, a pass whose run
// length reaches n copies.  What bounds it: at the sizes it is for (<= a few 10^5 rows, 28 bytes each) the records stay in the
// L2 / Infinity Cache, and a pass is bound by the LDS rank searches (11 dependent 28-byte compares per record) and by the launch
// chain (3 + passes launches), not by HBM: see the measurement in DESIGN 4.12.
//
// aggregate_matches: unique over pts1, gather pts2 through ia1, unique over that, composed gather of both sides -- a chain on the
// launcher above, n handed from stage to stage in device memory.
// The indexed estimateTransform (pcreg_dev_estimate_transform_indexed) is a kernel of ransac.hip, next to fit_moments / polar_to_T
// and the wave body of refine_by_distance_kernel it shares: those are file-local device functions.
#include "common.hpp"
#include "chunk_scan.hpp"

namespace pcreg {

namespace {

typedef unsigned long long u64;
constexpr int kUT = 2048;                            // records per tile of U1 and per output chunk of U2 .. U4
constexpr int kUBlock = 256;
constexpr int kUPer = kUT / kUBlock;                 // records per thread
static_assert((kUT & (kUT - 1)) == 0 && kUT % kUBlock == 0, "the bitonic network and the per-thread runs");
static_assert(kUT == kScanChunk && kUBlock == kScanBlock, "U3 / U4 are the chunk scan of chunk_scan.hpp");

struct RecBuf { u64* k0; u64* k1; u64* k2; uint32_t* row; };

__device__ __forceinline__ u64 key_of(double x) {
    u64 b = (u64)__double_as_longlong(x);
    if (b == 0x8000000000000000ull) b = 0;           // -0 orders as +0
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// (k0, k1, k2, row) of a before that of b
__device__ __forceinline__ bool rec_less(u64 a0, u64 a1, u64 a2, uint32_t ar, u64 b0, u64 b1, u64 b2, uint32_t br) {
    if (a0 != b0) return a0 < b0;
    if (a1 != b1) return a1 < b1;
    if (a2 != b2) return a2 < b2;
    return ar < br;
}
__device__ __forceinline__ int read_n(const int32_t* n_dev, int n_cap) { return max(0, min(*n_dev, n_cap)); }

// ---- U1 ---------------------------------------------------------------------------------------------------------------
// Padding records carry all-ones keys and row 0xFFFFFFFF: behind every real record (a real row is < 2^31), so the first
// min(T, n - base) records of the sorted tile are the real ones.
__global__ __launch_bounds__(kUBlock) void unique_tile_sort_kernel(const double* __restrict__ A, const int32_t* __restrict__ n_dev, int n_cap, int ld,
                                                                   RecBuf out) {
    __shared__ u64 s0[kUT], s1[kUT], s2[kUT];
    __shared__ uint32_t sr[kUT];
    const int n = read_n(n_dev, n_cap), base = blockIdx.x * kUT, tid = threadIdx.x;
    if (base >= n) return;
    for (int e = tid; e < kUT; e += kUBlock) {
        const int r = base + e;
        const bool live = r < n;
        s0[e] = live ? key_of(A[r]) : ~0ull;
        s1[e] = live ? key_of(A[r + (size_t)ld]) : ~0ull;
        s2[e] = live ? key_of(A[r + 2 * (size_t)ld]) : ~0ull;
        sr[e] = live ? (uint32_t)r : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int k = 2; k <= kUT; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int u = 0; u < kUPer / 2; ++u) {
                const int t = u * kUBlock + tid;
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const u64 a0 = s0[i], a1 = s1[i], a2 = s2[i], b0 = s0[l], b1 = s1[l], b2 = s2[l];
                const uint32_t ar = sr[i], br = sr[l];
                const bool ascending = (i & k) == 0;
                if (rec_less(b0, b1, b2, br, a0, a1, a2, ar) == ascending) {
                    s0[i] = b0; s1[i] = b1; s2[i] = b2; sr[i] = br;
                    s0[l] = a0; s1[l] = a1; s2[l] = a2; sr[l] = ar;
                }
            }
            __syncthreads();
        }
    }
    const int cnt = min(kUT, n - base);
    for (int e = tid; e < cnt; e += kUBlock) {
        out.k0[base + e] = s0[e]; out.k1[base + e] = s1[e]; out.k2[base + e] = s2[e]; out.row[base + e] = sr[e];
    }
}

// ---- U2 ---------------------------------------------------------------------------------------------------------------
// the number of records of run A among the first d records of merge(A, B): A = in[a_lo, a_lo + la), B = in[b_lo, b_lo + lb)
__device__ int merge_path_split(const RecBuf& in, int a_lo, int la, int b_lo, int lb, int d) {
    int lo = max(0, d - lb), hi = min(d, la);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int ia = a_lo + mid, ib = b_lo + (d - 1 - mid);                     // 0 <= mid < la, 0 <= d - 1 - mid < lb
        if (rec_less(in.k0[ia], in.k1[ia], in.k2[ia], in.row[ia], in.k0[ib], in.k1[ib], in.k2[ib], in.row[ib])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kUBlock) void unique_merge_kernel(RecBuf in, RecBuf out, const int32_t* __restrict__ n_dev, int n_cap, long long L) {
    __shared__ u64 s0[kUT], s1[kUT], s2[kUT];
    __shared__ uint32_t sr[kUT];
    __shared__ int s_split[2];
    const int n = read_n(n_dev, n_cap), tid = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * kUT;
    if (c0 >= n) return;
    const long long pb = c0 / (2 * L) * (2 * L);                                  // L is a multiple of the chunk: one pair per chunk
    const int a_lo = (int)pb, b_lo = (int)std::min<long long>(pb + L, n), b_hi = (int)std::min<long long>(pb + 2 * L, n);
    const int la = b_lo - a_lo, lb = b_hi - b_lo;
    const int d0 = (int)(c0 - pb), d1 = min(d0 + kUT, la + lb);
    if (tid < 2) s_split[tid] = merge_path_split(in, a_lo, la, b_lo, lb, tid == 0 ? d0 : d1);
    __syncthreads();
    const int a0 = s_split[0], a1 = s_split[1];
    const int b0 = d0 - a0, na = a1 - a0, nb = (d1 - a1) - b0, tot = na + nb;      // tot == d1 - d0 <= kUT
    for (int e = tid; e < tot; e += kUBlock) {
        const int g = e < na ? a_lo + a0 + e : b_lo + b0 + (e - na);
        s0[e] = in.k0[g]; s1[e] = in.k1[g]; s2[e] = in.k2[g]; sr[e] = in.row[g];
    }
    __syncthreads();
    for (int e = tid; e < tot; e += kUBlock) {
        const u64 x0 = s0[e], x1 = s1[e], x2 = s2[e];
        const uint32_t xr = sr[e];
        const bool from_a = e < na;
        int lo = from_a ? na : 0, hi = from_a ? tot : na;                          // the other side's records before this one
        const int side0 = lo;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rec_less(s0[mid], s1[mid], s2[mid], sr[mid], x0, x1, x2, xr)) lo = mid + 1;
            else hi = mid;
        }
        const int rank = (from_a ? e : e - na) + (lo - side0);
        const long long o = c0 + rank;                                             // < c0 + tot <= n
        out.k0[o] = x0; out.k1[o] = x1; out.k2[o] = x2; out.row[o] = xr;
    }
}

// ---- U3, U4 -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int is_head(const RecBuf& s, int i) {
    return i == 0 || s.k0[i] != s.k0[i - 1] || s.k1[i] != s.k1[i - 1] || s.k2[i] != s.k2[i - 1] ? 1 : 0;
}
__global__ __launch_bounds__(kUBlock) void unique_count_kernel(RecBuf s, const int32_t* __restrict__ n_dev, int n_cap, int32_t* __restrict__ csum) {
    const int n = read_n(n_dev, n_cap), base = blockIdx.x * kUT;
    if (base >= n) return;
    int32_t v = 0;
    for (int e = threadIdx.x; e < kUT; e += kUBlock) v += base + e < n ? is_head(s, base + e) : 0;
    chunk_sum(v, csum);
}
// thread t of chunk c owns records c * 2048 + 8 t .. + 7
__global__ __launch_bounds__(kUBlock) void unique_compact_kernel(RecBuf s, const int32_t* __restrict__ n_dev, int n_cap, const int32_t* __restrict__ csum,
                                                                 int32_t idx_base, int32_t* __restrict__ ia, int32_t* __restrict__ n_unique) {
    const int n = read_n(n_dev, n_cap), tid = threadIdx.x;
    if (n == 0) { if (blockIdx.x == 0 && tid == 0) *n_unique = 0; return; }
    if (blockIdx.x * kUT >= n) return;
    const int i0 = blockIdx.x * kUT + tid * kUPer;
    int32_t f[kUPer], mine = 0;
#pragma unroll
    for (int u = 0; u < kUPer; ++u) { f[u] = i0 + u < n ? is_head(s, i0 + u) : 0; mine += f[u]; }
    int32_t run = chunk_offset(csum, mine);
#pragma unroll
    for (int u = 0; u < kUPer; ++u) {
        if (f[u]) ia[run] = (int32_t)s.row[i0 + u] + idx_base;                     // run < the number of heads <= n
        run += f[u];
        if (i0 + u == n - 1) *n_unique = run;
    }
}

// ---- the gathers of aggregate_matches ---------------------------------------------------------------------------------
// dst(i, :) = src(idx[i], :), i < *n_dev (0-based idx; n x 3 column-major both sides)
__global__ __launch_bounds__(kUBlock) void gather_rows3_kernel(const double* __restrict__ src, int ld, const int32_t* __restrict__ idx,
                                                               const int32_t* __restrict__ n_dev, int n_cap, double* __restrict__ dst, int ldd) {
    const int n = read_n(n_dev, n_cap), i = blockIdx.x * kUBlock + threadIdx.x;
    if (i >= n) return;
    const int r = idx[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[i + (size_t)c * ldd] = src[r + (size_t)c * ld];
}
// j = ia1[ia2[i]]: out1(i, :) = pts1(j, :), out2(i, :) = pts2(j, :), ia[i] = j + idx_base
__global__ __launch_bounds__(kUBlock) void gather_composed_kernel(const double* __restrict__ p1, const double* __restrict__ p2, int ld,
                                                                  const int32_t* __restrict__ ia1, const int32_t* __restrict__ ia2,
                                                                  const int32_t* __restrict__ n_dev, int n_cap, double* __restrict__ out1,
                                                                  double* __restrict__ out2, int ldo, int32_t idx_base, int32_t* __restrict__ ia) {
    const int n = read_n(n_dev, n_cap), i = blockIdx.x * kUBlock + threadIdx.x;
    if (i >= n) return;
    const int j = ia1[ia2[i]];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out1[i + (size_t)c * ldo] = p1[j + (size_t)c * ld];
        out2[i + (size_t)c * ldo] = p2[j + (size_t)c * ld];
    }
    if (ia) ia[i] = j + idx_base;
}

// Workspace of unique_rows3: two record buffers (k0 | k1 | k2 | row, n each) and the heads per chunk of 2048 records:
// 2 * (3 * roundup(8 * max(n, 1), 256) + roundup(4 * max(n, 1), 256)) + roundup(4 * max(ceil(n / 2048), 1), 256) bytes
struct UniqueWs { RecBuf buf[2]; int32_t* csum; };
UniqueWs unique_ws_layout(int n_cap, void* base, size_t* bytes) {
    UniqueWs s{};
    const size_t nn = (size_t)(n_cap > 0 ? n_cap : 1);
    WsWalk w(base);
    for (int b = 0; b < 2; ++b) {
        s.buf[b].k0 = w.take<u64>(nn); s.buf[b].k1 = w.take<u64>(nn); s.buf[b].k2 = w.take<u64>(nn);
        s.buf[b].row = w.take<uint32_t>(nn);
    }
    s.csum = w.take<int32_t>((nn + kUT - 1) / kUT);
    *bytes = w.bytes();
    return s;
}
// Workspace of aggregate_matches: ia1, ia2 [n], n1 [1], pts2(ia1, :) [3 n], then unique_rows3's:
// 2 * roundup(4 * max(n, 1), 256) + 256 + roundup(24 * max(n, 1), 256) + unique_rows3_workspace(n) bytes
struct AggregateWs { int32_t* ia1; int32_t* ia2; int32_t* n1; double* p2g; void* uws; size_t uws_bytes; };
AggregateWs aggregate_ws_layout(int n_cap, void* base, size_t* bytes) {
    AggregateWs s{};
    const size_t nn = (size_t)(n_cap > 0 ? n_cap : 1);
    WsWalk w(base);
    s.ia1 = w.take<int32_t>(nn);
    s.ia2 = w.take<int32_t>(nn);
    s.n1 = w.take<int32_t>(1);
    s.p2g = w.take<double>(3 * nn);
    (void)unique_ws_layout(n_cap, nullptr, &s.uws_bytes);
    s.uws = w.take_bytes(s.uws_bytes);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t unique_rows3_ws_bytes(int n_cap) {
    size_t b; (void)unique_ws_layout(n_cap, nullptr, &b);
    return b;
}
size_t aggregate_matches_ws_bytes(int n_cap) {
    size_t b; (void)aggregate_ws_layout(n_cap, nullptr, &b);
    return b;
}

int launch_unique_rows3(const double* A, const int32_t* n_dev, int n_cap, int ld, int32_t idx_base, int32_t* ia, int32_t* n_unique, void* ws,
                        size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(n_dev && n_unique && n_cap >= 0 && n_cap <= 0x7FFFFFFF - kUT && ld >= n_cap && (n_cap == 0 || (A && ia)));
    size_t need;
    const UniqueWs s = unique_ws_layout(n_cap, ws, &need);
    PCREG_ARG(ws && ws_bytes >= need);
    const int chunks = (std::max(n_cap, 1) + kUT - 1) / kUT;
    const RecBuf* cur = &s.buf[0];
    const RecBuf* nxt = &s.buf[1];
    if (n_cap > 0) {
        hipLaunchKernelGGL(unique_tile_sort_kernel, dim3(chunks), dim3(kUBlock), 0, st, A, n_dev, n_cap, ld, *cur);
        for (long long L = kUT; L < n_cap; L *= 2) {
            hipLaunchKernelGGL(unique_merge_kernel, dim3(chunks), dim3(kUBlock), 0, st, *cur, *nxt, n_dev, n_cap, L);
            std::swap(cur, nxt);
        }
        hipLaunchKernelGGL(unique_count_kernel, dim3(chunks), dim3(kUBlock), 0, st, *cur, n_dev, n_cap, s.csum);
    }
    hipLaunchKernelGGL(unique_compact_kernel, dim3(chunks), dim3(kUBlock), 0, st, *cur, n_dev, n_cap, (const int32_t*)s.csum, idx_base, ia, n_unique);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

int launch_aggregate_matches(const double* pts1, const double* pts2, const int32_t* n_dev, int n_cap, int ld, double* out1, double* out2, int ldo,
                             int32_t idx_base, int32_t* ia, int32_t* n_out, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(n_dev && n_out && n_cap >= 0 && ld >= n_cap && ldo >= n_cap && (n_cap == 0 || (pts1 && pts2 && out1 && out2)));
    size_t need;
    const AggregateWs s = aggregate_ws_layout(n_cap, ws, &need);
    PCREG_ARG(ws && ws_bytes >= need);
    const int ldg = std::max(n_cap, 1), blocks = (n_cap + kUBlock - 1) / kUBlock;
    int rc = launch_unique_rows3(pts1, n_dev, n_cap, ld, 0, s.ia1, s.n1, s.uws, s.uws_bytes, st);          // [pts1, ia] = unique(pts1, 'rows')
    if (rc) return rc;
    if (n_cap > 0)                                                                                         // pts2 = pts2(ia, :)
        hipLaunchKernelGGL(gather_rows3_kernel, dim3(blocks), dim3(kUBlock), 0, st, pts2, ld, (const int32_t*)s.ia1, (const int32_t*)s.n1, n_cap, s.p2g, ldg);
    rc = launch_unique_rows3(s.p2g, s.n1, n_cap, ldg, 0, s.ia2, n_out, s.uws, s.uws_bytes, st);             // [pts2, ia] = unique(pts2, 'rows')
    if (rc) return rc;
    if (n_cap > 0)                                                                                         // pts1 = pts1(ia, :)
        hipLaunchKernelGGL(gather_composed_kernel, dim3(blocks), dim3(kUBlock), 0, st, pts1, pts2, ld, (const int32_t*)s.ia1, (const int32_t*)s.ia2,
                           (const int32_t*)n_out, n_cap, out1, out2, ldo, idx_base, ia);
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
