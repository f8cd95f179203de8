// pcreg_amd/csrc/knn_klist.hpp -- the k-list of the exact k-nearest walks (knn_k.hip, knn_normals.hip, knn_denoise.hip): a sorted list of KB
// (distance, row) pairs in registers, ordered by (distance, row) with the empty entry (-1) last; insertion, the k-th entry,
// and the merge with a partner lane's list; and the host's dispatch from k to KB (klist_dispatch).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace pcreg {
namespace {

// The one dispatch on the list size that serves k: f(std::integral_constant<int, KB>{}) with KB the smallest of KB_MIN, 2 KB_MIN,
// .., 32 that is >= k (k <= PCREG_KNN_MAX_K = 32).  Only those sizes are instantiated.
template <int KB_MIN, class F>
inline void klist_dispatch(int k, F&& f) {
    if constexpr (KB_MIN >= 32) f(std::integral_constant<int, 32>{});
    else if (k <= KB_MIN) f(std::integral_constant<int, KB_MIN>{});
    else klist_dispatch<2 * KB_MIN>(k, f);
}

__device__ __forceinline__ bool knn_k_lt(float da, int ia, float db, int ib) {     // (distance, row); -1 (empty) sorts last
    return da < db || (da == db && (unsigned)ia < (unsigned)ib);
}
// sorted insertion by a KB-stage compare-exchange chain (an entry that beats none falls off the end)
template <int KB>
__device__ __forceinline__ void klist_insert(float (&ld)[KB], int (&li)[KB], float d, int j) {
    float x = d; int xi = j;
#pragma unroll
    for (int s = 0; s < KB; ++s) {
        const bool lt = knn_k_lt(x, xi, ld[s], li[s]);
        const float lo = lt ? x : ld[s], hi = lt ? ld[s] : x;
        const int loi = lt ? xi : li[s], hii = lt ? li[s] : xi;
        ld[s] = lo; li[s] = loi; x = hi; xi = hii;
    }
}
template <int KB>
__device__ __forceinline__ float klist_kth(const float (&ld)[KB], int k) {
    float v = ld[0];
#pragma unroll
    for (int s = 1; s < KB; ++s) v = s == k - 1 ? ld[s] : v;
    return v;
}
// the KB smallest of two sorted lists (the partner lane's arrives by xor shuffle): c_s = min(a_s, b_{KB-1-s}) is bitonic,
// a half-cleaner cascade sorts it; both lanes of the pair end with the same list
template <int KB>
__device__ __forceinline__ void klist_merge_xor(float (&ld)[KB], int (&li)[KB], int o) {
    float od[KB]; int oi[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) { od[s] = __shfl_xor(ld[s], o); oi[s] = __shfl_xor(li[s], o); }
#pragma unroll
    for (int s = 0; s < KB; ++s) {
        if (knn_k_lt(od[KB - 1 - s], oi[KB - 1 - s], ld[s], li[s])) { ld[s] = od[KB - 1 - s]; li[s] = oi[KB - 1 - s]; }
    }
#pragma unroll
    for (int h = KB / 2; h > 0; h >>= 1) {
#pragma unroll
        for (int s = 0; s < KB; ++s) {
            if ((s & h) == 0) {
                const bool sw = knn_k_lt(ld[s + h], li[s + h], ld[s], li[s]);
                const float a = sw ? ld[s + h] : ld[s], b = sw ? ld[s] : ld[s + h];
                const int ia = sw ? li[s + h] : li[s], ib = sw ? li[s] : li[s + h];
                ld[s] = a; ld[s + h] = b; li[s] = ia; li[s + h] = ib;
            }
        }
    }
}

// The same two on distances ALONE, for a walk that needs the multiset of the k smallest distances and not their rows
// (knn_denoise.hip): half the list registers; equal distances are interchangeable, so no tie rule is needed.
template <int KB>
__device__ __forceinline__ void klist_insert(float (&ld)[KB], float d) {
    float x = d;
#pragma unroll
    for (int s = 0; s < KB; ++s) {
        const float lo = fminf(x, ld[s]), hi = fmaxf(x, ld[s]);
        ld[s] = lo; x = hi;
    }
}
// a bitonic list into ascending order: the half-cleaner cascade
template <int KB>
__device__ __forceinline__ void klist_sort_bitonic(float (&ld)[KB]) {
#pragma unroll
    for (int h = KB / 2; h > 0; h >>= 1) {
#pragma unroll
        for (int s = 0; s < KB; ++s) {
            if ((s & h) == 0) {
                const float a = fminf(ld[s], ld[s + h]), b = fmaxf(ld[s], ld[s + h]);
                ld[s] = a; ld[s + h] = b;
            }
        }
    }
}
template <int KB>
__device__ __forceinline__ void klist_merge_xor(float (&ld)[KB], int o) {
    float od[KB];
#pragma unroll
    for (int s = 0; s < KB; ++s) od[s] = __shfl_xor(ld[s], o);
#pragma unroll
    for (int s = 0; s < KB; ++s) ld[s] = fminf(ld[s], od[KB - 1 - s]);
    klist_sort_bitonic<KB>(ld);
}

}  // namespace
}  // namespace pcreg
