// pcreg_amd/csrc/downsample.hip -- pcdownsample(pc, 'gridAverage', step) for n x 3 fp32 rows on the device: the mean of the rows of
// every occupied grid cell.  The contract is pcreg_downsample_grid_f32's (include/pcreg.h); DESIGN 4.17.
//
// A call is one launch chain; nothing is read on the host, no kernel waits for another workgroup, every loop has a trip count
// fixed by n or by a constant.  T = 2048 records per workgroup throughout (the chunk of chunk_scan.hpp).
//   D1  ds_limits_partial_kernel  lo / hi of every coordinate and the number of live rows per chunk of T rows (a row is live
//                                 when its three coordinates are finite)
//   D2  ds_limits_final_kernel    one workgroup: the partials reduced; thread 0 derives the largest cell index per axis, the
//                                 three bit widths, the refusal word, the used key bits and the live sort passes -> the header
//   D3  ds_keys_kernel            (u64 key, u32 row) per row into buffer 0.  key = c0 << (w1 + w2) | c1 << w2 | c2 (<= 63 bits);
//                                 a dead row's key is all ones
//   D4  per pass p = 0 .. 7 over the 8-bit digit at bit 8 p, three launches:
//         ds_hist_kernel          the digit histogram of every chunk, hist[digit][chunk]
//         ds_scan_kernel          workgroup d: the exclusive scan of hist[d][.] over the chunks in place, and total[d]
//         ds_scatter_kernel       the chunk's records leave for out[base(digit) + hist[digit][chunk] + rank]: rank is the number
//                                 of records of the same digit before it IN THE CHUNK, found per round of 256 records by a wave
//                                 match (eight ballots), the counts of the waves before it (LDS) and the rounds before it, so
//                                 the sort is stable by construction and equal keys stay in ascending row order.  The records
//                                 are first put in (digit, rank) order in LDS (24 KB) and written from there, so that
//                                 neighbouring threads write neighbouring records of a digit
//       The used key bits are B = w0 + w1 + w2, plus the bit above them when the cloud has a dead row (that bit is what puts
//       the all-ones keys behind every live one); passes = ceil(used / 8) is in the header.  A pass p >= passes does NOTHING:
//       pass p reads buffer p & 1 and writes the other, so the sorted records lie in buffer passes & 1, which D5 .. D7 pick from
//       the header -- the launcher's chain does not depend on the data, and a dead pass moves no byte.
//   D5  ds_heads_count_kernel     heads per chunk: record i < n_live whose key differs from record i - 1's (or i = 0)
//   D6  ds_heads_compact_kernel   the chunk scan (chunk_scan.hpp): head number v starts at record vstart[v]; the chunk that holds
//                                 record n - 1 writes n_out
//   D7  ds_means_kernel           thread v < n_out walks records vstart[v] .. vstart[v + 1] (n_live for the last) in order: rows
//                                 gathered eight at a time ahead of the adds, three double sums from 0.0 in record (= ascending
//                                 row) order, one division, one rounding; count, and label of every member.  Thread i >= n_live
//                                 writes label 0 for dead record i.
// A refused cloud (an axis with 2^21 cells or more: info = 1) and a cloud without a live row stop after D2: D3 .. D7 return at
// once, D6 writes n_out = 0.  The result is a function of (pts, step): integer LDS atomics in the histogram only (a count does
// not depend on their order), no floating-point atomic, and every workspace word that is read was written by this call.
#include "common.hpp"
#include "chunk_scan.hpp"
#include <cmath>

namespace pcreg {

namespace {

typedef unsigned long long u64;
constexpr int kDsT = 2048;                           // records per workgroup of every kernel here (tests/test_gpu_downsample.py: T)
constexpr int kDsBlock = 256;
constexpr int kDsPer = kDsT / kDsBlock;              // rounds of the scatter; records per thread
constexpr int kDsPasses = 8;                         // 8-bit digits of a 64-bit key
constexpr double kDsMaxCells = 2097152.0;            // 2^21: a cell index at or above it refuses the cloud
static_assert(kDsT == kScanChunk && kDsBlock == kScanBlock, "D5 / D6 are the chunk scan of chunk_scan.hpp");

typedef VoxelHdr DsHdr;                             // (common.hpp: the NDT table's chain reads it too)

__device__ __forceinline__ bool ds_live(float x, float y, float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;       // (false for NaN)
}
// the cell of a live coordinate: IEEE subtraction and division in double (the file is built without contraction)
__device__ __forceinline__ double ds_cell(float x, float lo, double step) { return floor(((double)x - (double)lo) / step); }
__device__ __forceinline__ bool ds_idle(const DsHdr* h) { return h->info != 0 || h->n_live == 0; }

// ---- D1, D2 -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDsBlock) void ds_limits_partial_kernel(const float* __restrict__ pts, int n, int ld, float* __restrict__ part,
                                                                     int32_t* __restrict__ live_cnt) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int32_t cnt = 0;
    const int base = blockIdx.x * kDsT;
#pragma unroll
    for (int u = 0; u < kDsPer; ++u) {
        const int r = base + u * kDsBlock + threadIdx.x;
        if (r < n) {
            const float v[3] = {pts[r], pts[r + (size_t)ld], pts[r + 2 * (size_t)ld]};
            if (ds_live(v[0], v[1], v[2])) {
                ++cnt;
#pragma unroll
                for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], v[c]); hi[c] = fmaxf(hi[c], v[c]); }
            }
        }
    }
    __shared__ float s[kDsBlock / 64][6];
    __shared__ int32_t sc[kDsBlock / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
        cnt += __shfl_xor(cnt, o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[threadIdx.x >> 6][c] = lo[c]; s[threadIdx.x >> 6][3 + c] = hi[c]; }
        sc[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = s[0][threadIdx.x];
        for (int w = 1; w < kDsBlock / 64; ++w) v = threadIdx.x < 3 ? fminf(v, s[w][threadIdx.x]) : fmaxf(v, s[w][threadIdx.x]);
        part[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
    if (threadIdx.x == 6) live_cnt[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
}

__global__ __launch_bounds__(kDsBlock) void ds_limits_final_kernel(const float* __restrict__ part, const int32_t* __restrict__ live_cnt, int nparts,
                                                                   int n, double step, DsHdr* __restrict__ hdr, int32_t* __restrict__ info_out) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int32_t cnt = 0;
    for (int b = threadIdx.x; b < nparts; b += kDsBlock) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], part[(size_t)b * 6 + c]); hi[c] = fmaxf(hi[c], part[(size_t)b * 6 + 3 + c]); }
        cnt += live_cnt[b];
    }
    __shared__ float s[kDsBlock / 64][6];
    __shared__ int32_t sc[kDsBlock / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
        cnt += __shfl_xor(cnt, o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s[threadIdx.x >> 6][c] = lo[c]; s[threadIdx.x >> 6][3 + c] = hi[c]; }
        sc[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    DsHdr h{};
    for (int w = 0; w < kDsBlock / 64; ++w) {
        for (int c = 0; c < 3; ++c) {
            h.lo[c] = w ? fminf(h.lo[c], s[w][c]) : s[0][c];
            h.hi[c] = w ? fmaxf(h.hi[c], s[w][3 + c]) : s[0][3 + c];
        }
        h.n_live += sc[w];
    }
    int bits = 0;
    if (h.n_live > 0) {
        // the cell index is monotone in the coordinate, so the largest one is hi's
        for (int c = 0; c < 3; ++c) {
            const double cmax = ds_cell(h.hi[c], h.lo[c], step);
            if (!(cmax < kDsMaxCells)) { h.info = 1; continue; }
            int w = 0;
            for (long long v = (long long)cmax; v > 0; v >>= 1) ++w;
            h.w[c] = w;
            bits += w;
        }
    }
    h.used = bits + (h.n_live < n ? 1 : 0);
    h.passes = (h.used + 7) / 8;
    *hdr = h;
    *info_out = h.info;
}

// ---- D3 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDsBlock) void ds_keys_kernel(const float* __restrict__ pts, int n, int ld, double step, const DsHdr* __restrict__ hdr,
                                                           u64* __restrict__ key, uint32_t* __restrict__ row) {
    if (ds_idle(hdr)) return;
    const int r = blockIdx.x * kDsBlock + threadIdx.x;
    if (r >= n) return;
    const float x = pts[r], y = pts[r + (size_t)ld], z = pts[r + 2 * (size_t)ld];
    u64 k = ~0ull;
    if (ds_live(x, y, z)) {
        const u64 c0 = (u64)(long long)ds_cell(x, hdr->lo[0], step), c1 = (u64)(long long)ds_cell(y, hdr->lo[1], step),
                  c2 = (u64)(long long)ds_cell(z, hdr->lo[2], step);
        k = (((c0 << hdr->w[1]) | c1) << hdr->w[2]) | c2;
    }
    key[r] = k;
    row[r] = (uint32_t)r;
}

// ---- D4 ---------------------------------------------------------------------------------------------------------------
struct DsBuf { u64* key; uint32_t* row; };

__global__ __launch_bounds__(kDsBlock) void ds_hist_kernel(DsBuf b0, DsBuf b1, int n, int pass, int chunks, const DsHdr* __restrict__ hdr,
                                                           uint32_t* __restrict__ hist) {
    if (ds_idle(hdr) || pass >= hdr->passes) return;
    const u64* __restrict__ key = (pass & 1) ? b1.key : b0.key;
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * kDsT, shift = 8 * pass;
#pragma unroll
    for (int u = 0; u < kDsPer; ++u) {
        const int i = base + u * kDsBlock + threadIdx.x;
        if (i < n) atomicAdd(&s_h[(unsigned)(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * chunks + blockIdx.x] = s_h[threadIdx.x];
}

// workgroup d: hist[d][0 .. chunks) becomes its exclusive scan, total[d] its sum.  Thread t owns `per` consecutive chunks.
__global__ __launch_bounds__(kDsBlock) void ds_scan_kernel(int pass, int chunks, const DsHdr* __restrict__ hdr, uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ total) {
    if (ds_idle(hdr) || pass >= hdr->passes) return;
    __shared__ uint32_t s_thr[kDsBlock];
    uint32_t* __restrict__ h = hist + (size_t)blockIdx.x * chunks;
    const int tid = threadIdx.x, per = (chunks + kDsBlock - 1) / kDsBlock;
    const int c0 = min(tid * per, chunks), c1 = min(c0 + per, chunks);
    uint32_t mine = 0;
    for (int c = c0; c < c1; ++c) mine += h[c];
    s_thr[tid] = mine;
    __syncthreads();
    for (int o = 1; o < kDsBlock; o <<= 1) {
        const uint32_t add = tid >= o ? s_thr[tid - o] : 0;
        __syncthreads();
        s_thr[tid] += add;
        __syncthreads();
    }
    uint32_t run = s_thr[tid] - mine;
    for (int c = c0; c < c1; ++c) { const uint32_t v = h[c]; h[c] = run; run += v; }
    if (tid == kDsBlock - 1) total[blockIdx.x] = s_thr[tid];
}

__global__ __launch_bounds__(kDsBlock) void ds_scatter_kernel(DsBuf b0, DsBuf b1, int n, int pass, int chunks, const DsHdr* __restrict__ hdr,
                                                              const uint32_t* __restrict__ hist, const uint32_t* __restrict__ total) {
    if (ds_idle(hdr) || pass >= hdr->passes) return;
    const DsBuf in = (pass & 1) ? b1 : b0, out = (pass & 1) ? b0 : b1;
    __shared__ u64 s_key[kDsT];                      // the chunk's records ordered by (digit, place in the chunk)
    __shared__ uint32_t s_row[kDsT];
    __shared__ uint32_t s_cnt[256];                  // the chunk's records of every digit, then where its next one goes in s_key
    __shared__ uint32_t s_lstart[256];               // where the digit's records start in s_key
    __shared__ uint32_t s_gbase[256];                // where the chunk's first record of the digit goes in the output
    __shared__ uint32_t s_wcnt[kDsBlock / 64][256];  // this round's records of every digit per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = blockIdx.x * kDsT, shift = 8 * pass;
    u64 k[kDsPer]; uint32_t r[kDsPer];
    s_cnt[tid] = 0;
    s_gbase[tid] = total[tid];
#pragma unroll
    for (int w = 0; w < kDsBlock / 64; ++w) s_wcnt[w][tid] = 0;
#pragma unroll
    for (int u = 0; u < kDsPer; ++u) {
        const int i = base + u * kDsBlock + tid;
        k[u] = i < n ? in.key[i] : 0ull;
        r[u] = i < n ? in.row[i] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kDsPer; ++u)
        if (base + u * kDsBlock + tid < n) atomicAdd(&s_cnt[(unsigned)(k[u] >> shift) & 255u], 1u);
    __syncthreads();
    // two exclusive scans over the 256 digits: the chunk's counts (places in s_key) and the totals (the digit's base in the output)
    const uint32_t cnt = s_cnt[tid], tot = s_gbase[tid];
    for (int o = 1; o < 256; o <<= 1) {
        const uint32_t a = tid >= o ? s_cnt[tid - o] : 0, b = tid >= o ? s_gbase[tid - o] : 0;
        __syncthreads();
        s_cnt[tid] += a; s_gbase[tid] += b;
        __syncthreads();
    }
    const uint32_t lstart = s_cnt[tid] - cnt;
    __syncthreads();
    s_cnt[tid] = lstart;
    s_lstart[tid] = lstart;
    s_gbase[tid] = (s_gbase[tid] - tot) + hist[(size_t)tid * chunks + blockIdx.x];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kDsPer; ++u) {                // (the trip count is uniform: every thread reaches every barrier)
        const bool on = base + u * kDsBlock + tid < n;
        const unsigned d = (unsigned)(k[u] >> shift) & 255u;
        // the lanes of this wave with the same digit
        u64 peers = __ballot(on);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 m = __ballot(on && ((d >> b) & 1u));
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (on && rank == 0) s_wcnt[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (on) {
            uint32_t o = s_cnt[d] + (uint32_t)rank;
            for (int w = 0; w < wave; ++w) o += s_wcnt[w][d];
            s_key[o] = k[u];                         // o < the chunk's records <= kDsT
            s_row[o] = r[u];
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int w = 0; w < kDsBlock / 64; ++w) { add += s_wcnt[w][tid]; s_wcnt[w][tid] = 0; }
        s_cnt[tid] += add;
        __syncthreads();
    }
    // out: neighbouring threads write neighbouring records of a digit
    const int m = min(kDsT, n - base);
    for (int j = tid; j < m; j += kDsBlock) {
        const u64 kj = s_key[j];
        const unsigned d = (unsigned)(kj >> shift) & 255u;
        const uint32_t o = s_gbase[d] + ((uint32_t)j - s_lstart[d]);     // o < n: the places of all records are a permutation of 0 .. n - 1
        out.key[o] = kj;
        out.row[o] = s_row[j];
    }
}

// ---- D5, D6 -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ds_is_head(const u64* __restrict__ key, int i, int n_live) {
    return i < n_live && (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}
__global__ __launch_bounds__(kDsBlock) void ds_heads_count_kernel(DsBuf b0, DsBuf b1, const DsHdr* __restrict__ hdr, int32_t* __restrict__ csum) {
    if (ds_idle(hdr)) return;
    const u64* __restrict__ key = (hdr->passes & 1) ? b1.key : b0.key;
    const int n_live = hdr->n_live, base = blockIdx.x * kDsT;
    int32_t v = 0;
    for (int e = threadIdx.x; e < kDsT; e += kDsBlock) v += ds_is_head(key, base + e, n_live);
    chunk_sum(v, csum);
}
// thread t of chunk c owns records c * 2048 + 8 t .. + 7
__global__ __launch_bounds__(kDsBlock) void ds_heads_compact_kernel(DsBuf b0, DsBuf b1, int n, const DsHdr* __restrict__ hdr,
                                                                    const int32_t* __restrict__ csum, int32_t* __restrict__ vstart,
                                                                    int32_t* __restrict__ n_out) {
    if (ds_idle(hdr)) { if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = 0; return; }
    const u64* __restrict__ key = (hdr->passes & 1) ? b1.key : b0.key;
    const int n_live = hdr->n_live, i0 = blockIdx.x * kDsT + threadIdx.x * kDsPer;
    int32_t f[kDsPer], mine = 0;
#pragma unroll
    for (int u = 0; u < kDsPer; ++u) { f[u] = ds_is_head(key, i0 + u, n_live); mine += f[u]; }
    int32_t run = chunk_offset(csum, mine);
#pragma unroll
    for (int u = 0; u < kDsPer; ++u) {
        if (f[u]) vstart[run] = i0 + u;                // run < the number of heads <= n
        run += f[u];
        if (i0 + u == n - 1) *n_out = run;
    }
}

// ---- D7 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDsBlock) void ds_means_kernel(const float* __restrict__ pts, int n, int ld, DsBuf b0, DsBuf b1,
                                                            const DsHdr* __restrict__ hdr, const int32_t* __restrict__ vstart,
                                                            const int32_t* __restrict__ n_out_dev, float* __restrict__ out, int ldo,
                                                            int32_t* __restrict__ count, int32_t* __restrict__ label) {
    if (ds_idle(hdr)) return;
    const uint32_t* __restrict__ row = (hdr->passes & 1) ? b1.row : b0.row;
    const int n_live = hdr->n_live, n_out = *n_out_dev;
    const int v = blockIdx.x * kDsBlock + threadIdx.x;
    if (v >= n) return;
    if (label && v >= n_live) label[row[v]] = 0;       // record v is a dead row's
    if (v >= n_out) return;
    const int s = vstart[v], e = v + 1 < n_out ? vstart[v + 1] : n_live;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = s; i < e; i += 8) {
        // the batch's rows, then their gathers, are issued ahead of the adds that consume them; a slot past the run loads nothing
        float x[8], y[8], z[8];
        uint32_t r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = i + u < e ? row[i + u] : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            x[u] = y[u] = z[u] = 0.0f;
            if (i + u < e) {
                x[u] = pts[r[u]]; y[u] = pts[r[u] + (size_t)ld]; z[u] = pts[r[u] + 2 * (size_t)ld];
                if (label) label[r[u]] = v + 1;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool on = i + u < e;
            sx = on ? sx + (double)x[u] : sx; sy = on ? sy + (double)y[u] : sy; sz = on ? sz + (double)z[u] : sz;
        }
    }
    const double dn = (double)(e - s);
    out[v] = (float)(sx / dn);
    out[v + (size_t)ldo] = (float)(sy / dn);
    out[v + 2 * (size_t)ldo] = (float)(sz / dn);
    if (count) count[v] = e - s;
}

// Workspace, with nn = max(n, 1) and chunks = ceil(nn / 2048): the header (256 bytes), the limits' partials (6 floats and one
// count per chunk), two record buffers (u64 key | u32 row, nn each), the digit histogram [256][chunks] and its totals [256],
// the heads per chunk, the first record of every voxel [nn]:
//   256 + roundup(24 * chunks, 256) + roundup(4 * chunks, 256) + 2 * (roundup(8 * nn, 256) + roundup(4 * nn, 256))
//       + roundup(1024 * chunks, 256) + 1024 + roundup(4 * chunks, 256) + roundup(4 * nn, 256) bytes
struct DownsampleWs { DsHdr* hdr; float* part; int32_t* live_cnt; DsBuf buf[2]; uint32_t* hist; uint32_t* total; int32_t* csum; int32_t* vstart; };
DownsampleWs downsample_ws_layout(int n, void* base, size_t* bytes) {
    static_assert(sizeof(DsHdr) <= 256, "the header's slot");
    DownsampleWs s{};
    const size_t nn = (size_t)(n > 0 ? n : 1), chunks = (nn + kDsT - 1) / kDsT;
    WsWalk w(base);
    s.hdr = (DsHdr*)w.take_bytes(256);
    s.part = w.take<float>(6 * chunks);
    s.live_cnt = w.take<int32_t>(chunks);
    for (int b = 0; b < 2; ++b) { s.buf[b].key = w.take<u64>(nn); s.buf[b].row = w.take<uint32_t>(nn); }
    s.hist = w.take<uint32_t>(256 * chunks);
    s.total = w.take<uint32_t>(256);
    s.csum = w.take<int32_t>(chunks);
    s.vstart = w.take<int32_t>(nn);
    *bytes = w.bytes();
    return s;
}

}  // namespace

size_t downsample_grid_ws_bytes(int n) {
    size_t b; (void)downsample_ws_layout(n, nullptr, &b);
    return b;
}
int downsample_grid_chunk() { return kDsT; }

// D1 .. D6: the chain up to the first record of every voxel.  *order (may be null) names what D7 -- or another consumer of the voxel
// order (ndt.hip) -- reads: the header, the two row buffers of which the header's passes & 1 picks the sorted one, vstart
int launch_voxel_order(const float* pts, int n, int ld, double step, int32_t* n_out, int32_t* info, void* ws, size_t ws_bytes, hipStream_t st,
                       VoxelOrder* order) {
    PCREG_ARG(n >= 0 && n <= 0x7FFFFFFF - kDsT && ld >= n && std::isfinite(step) && step > 0.0 && n_out && info && (n == 0 || pts));
    size_t need;
    const DownsampleWs s = downsample_ws_layout(n, ws, &need);
    PCREG_ARG(ws && ws_bytes >= need);
    const int chunks = (std::max(n, 1) + kDsT - 1) / kDsT, nparts = n > 0 ? chunks : 0;
    const dim3 grid(chunks), block(kDsBlock), rows((std::max(n, 1) + kDsBlock - 1) / kDsBlock);
    if (n > 0) hipLaunchKernelGGL(ds_limits_partial_kernel, grid, block, 0, st, pts, n, ld, s.part, s.live_cnt);
    hipLaunchKernelGGL(ds_limits_final_kernel, dim3(1), block, 0, st, (const float*)s.part, (const int32_t*)s.live_cnt, nparts, n, step, s.hdr, info);
    if (n > 0) {
        hipLaunchKernelGGL(ds_keys_kernel, rows, block, 0, st, pts, n, ld, step, (const DsHdr*)s.hdr, s.buf[0].key, s.buf[0].row);
        for (int p = 0; p < kDsPasses; ++p) {
            hipLaunchKernelGGL(ds_hist_kernel, grid, block, 0, st, s.buf[0], s.buf[1], n, p, chunks, (const DsHdr*)s.hdr, s.hist);
            hipLaunchKernelGGL(ds_scan_kernel, dim3(256), block, 0, st, p, chunks, (const DsHdr*)s.hdr, s.hist, s.total);
            hipLaunchKernelGGL(ds_scatter_kernel, grid, block, 0, st, s.buf[0], s.buf[1], n, p, chunks, (const DsHdr*)s.hdr, (const uint32_t*)s.hist,
                               (const uint32_t*)s.total);
        }
        hipLaunchKernelGGL(ds_heads_count_kernel, grid, block, 0, st, s.buf[0], s.buf[1], (const DsHdr*)s.hdr, s.csum);
    }
    hipLaunchKernelGGL(ds_heads_compact_kernel, grid, block, 0, st, s.buf[0], s.buf[1], n, (const DsHdr*)s.hdr, (const int32_t*)s.csum, s.vstart, n_out);
    PCREG_HIP(hipGetLastError());
    if (order) *order = VoxelOrder{s.hdr, {s.buf[0].row, s.buf[1].row}, s.vstart};
    return PCREG_OK;
}

int launch_downsample_grid(const float* pts, int n, int ld, double step, float* out, int ldo, int32_t* count, int32_t* label, int32_t* n_out,
                           int32_t* info, void* ws, size_t ws_bytes, hipStream_t st) {
    PCREG_ARG(n >= 0 && n <= 0x7FFFFFFF - kDsT && ld >= n && ldo >= n && std::isfinite(step) && step > 0.0 && n_out && info &&
              (n == 0 || (pts && out)));
    const int rc = launch_voxel_order(pts, n, ld, step, n_out, info, ws, ws_bytes, st, nullptr);
    if (rc) return rc;
    if (n > 0) {
        size_t need;
        const DownsampleWs s = downsample_ws_layout(n, ws, &need);
        const dim3 block(kDsBlock), rows((n + kDsBlock - 1) / kDsBlock);
        hipLaunchKernelGGL(ds_means_kernel, rows, block, 0, st, pts, n, ld, s.buf[0], s.buf[1], (const DsHdr*)s.hdr, (const int32_t*)s.vstart,
                           (const int32_t*)n_out, out, ldo, count, label);
    }
    PCREG_HIP(hipGetLastError());
    return PCREG_OK;
}

}  // namespace pcreg
