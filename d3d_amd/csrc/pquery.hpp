// pquery.hpp -- what the neighbour searches of the point branch share: psample.hip (k_ball_query, k_knn_query: the whole segment per
// centre) and pgrid.hip (their grid-accelerated siblings: only the cells a centre can reach).  The segment search, q, the
// order-keeping key of a candidate and its insertion into the keys a wavefront holds sorted across its lanes.  One definition of
// each, so the two routes cannot drift apart: their tables are equal bit for bit by construction of q and of the order.
#pragma once
#include "common.hpp"

#include <cmath>
#include <limits>

namespace {

template <typename T> __device__ __forceinline__ bool ps_finite3(T x, T y, T z)
{
    const T inf = std::numeric_limits<T>::infinity();
    return fabs(x) < inf && fabs(y) < inf && fabs(z) < inf;         // false for NaN
}

// the segment b of centre c: center_offsets[b] <= c < center_offsets[b + 1] (the last such b where segments are empty)
__device__ __forceinline__ int64_t ps_segment_of(const int64_t *__restrict__ center_offsets, int64_t segments, int64_t c)
{
    int64_t lo = 0, hi = segments;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (center_offsets[mid] <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

// q(i, c) of include/d3d_hip.h: every operation one rounding in T (the build does not contract)
template <typename T> __device__ __forceinline__ T ps_q(T px, T py, T pz, T cx, T cy, T cz)
{
    const T dx = px - cx, dy = py - cy, dz = pz - cz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// ---------------------------------------------------------------- the key of a candidate
// The order-keeping key of a candidate: q >= +0 always, so its bits order as unsigned integers; the row breaks ties (the lower row
// first).  fp32: one 64-bit word {q bits : 32 | row : 32}; fp64: the 64 bits of q and the row beside them.  All ones = "no entry":
// above every candidate (its q bits would be a NaN's, and a NaN q is no candidate).  A uint32_t is the key "row alone" (the grid
// ball query: the lowest rows), all ones = "no entry" as well.
struct KnnKey64 {
    uint64_t d;
    uint32_t row;
};
template <typename T> struct KnnKeyOf;
template <> struct KnnKeyOf<float> { typedef uint64_t type; };
template <> struct KnnKeyOf<double> { typedef KnnKey64 type; };

__device__ __forceinline__ uint64_t knn_make(float q, uint32_t row) { return ((uint64_t)__float_as_uint(q) << 32) | row; }
__device__ __forceinline__ KnnKey64 knn_make(double q, uint32_t row) { return KnnKey64{(uint64_t)__double_as_longlong(q), row}; }
__device__ __forceinline__ void knn_clear(uint32_t &k) { k = ~0u; }
__device__ __forceinline__ void knn_clear(uint64_t &k) { k = ~0ull; }
__device__ __forceinline__ void knn_clear(KnnKey64 &k) { k.d = ~0ull, k.row = ~0u; }
__device__ __forceinline__ bool knn_lt(uint32_t a, uint32_t b) { return a < b; }
__device__ __forceinline__ bool knn_lt(uint64_t a, uint64_t b) { return a < b; }
__device__ __forceinline__ bool knn_lt(const KnnKey64 &a, const KnnKey64 &b) { return a.d < b.d || (a.d == b.d && a.row < b.row); }
__device__ __forceinline__ bool knn_none(uint32_t k) { return k == ~0u; }
__device__ __forceinline__ bool knn_none(uint64_t k) { return k == ~0ull; }
__device__ __forceinline__ bool knn_none(const KnnKey64 &k) { return k.d == ~0ull; }
__device__ __forceinline__ uint32_t knn_row(uint64_t k) { return (uint32_t)k; }
__device__ __forceinline__ uint32_t knn_row(const KnnKey64 &k) { return k.row; }
__device__ __forceinline__ float knn_dist(uint64_t k, float) { return __uint_as_float((uint32_t)(k >> 32)); }
__device__ __forceinline__ double knn_dist(const KnnKey64 &k, double) { return __longlong_as_double((long long)k.d); }
__device__ __forceinline__ uint32_t knn_readlane(uint32_t k, int lane) { return wave_readlane(k, lane); }
__device__ __forceinline__ uint64_t knn_readlane(uint64_t k, int lane) { return wave_readlane(k, lane); }
__device__ __forceinline__ KnnKey64 knn_readlane(const KnnKey64 &k, int lane) { return KnnKey64{wave_readlane(k.d, lane), wave_readlane(k.row, lane)}; }
// lane l reads lane l - 1 over the whole wavefront (wave_shr:1); lane 0 reads 0 and is never asked
__device__ __forceinline__ uint32_t knn_up(uint32_t k) { return d3d_dpp_u32<0x138, 0xf>(k); }
__device__ __forceinline__ uint64_t knn_up(uint64_t k) { return d3d_dpp_u64<0x138, 0xf>(k); }
__device__ __forceinline__ KnnKey64 knn_up(const KnnKey64 &k) { return KnnKey64{d3d_dpp_u64<0x138, 0xf>(k.d), d3d_dpp_u32<0x138, 0xf>(k.row)}; }

// One tile of 64 keys (one per lane; all ones where the lane has none) against the keys the wavefront holds SORTED ACROSS ITS LANES:
// lane l the l-th smallest (all ones while fewer than l + 1 were seen), tau = lane k - 1's key, wave-uniform, is what a key has to
// beat.  Every lane whose key beats tau, in ascending lane, is inserted wave-uniformly: the key is broadcast, its position is the
// number of held keys below it, the lanes above take their lower neighbour's key (one wave shift), the lane at the position takes
// the new key, tau is read again and the ballot is taken again over the lanes above.  All 64 lanes call it.
template <typename K> __device__ __forceinline__ void knn_insert_tile(const K &key, K &held, K &tau, int lane, int k)
{
    unsigned long long vote = __ballot(knn_lt(key, tau));
    while (vote) {                             // (wave-uniform)
        const int src = __ffsll((long long)vote) - 1;
        const K nk = knn_readlane(key, src);
        const int pos = __popcll(__ballot(knn_lt(held, nk)));                   // held is sorted: the lanes 0 .. pos - 1
        const K up = knn_up(held);
        if (lane > pos) held = up;
        else if (lane == pos) held = nk;
        tau = knn_readlane(held, k - 1);
        // the lanes above src that still beat tau, which has come down: of a tile's 64 rows only a few are ever inserted
        vote = __ballot(knn_lt(key, tau)) & (~1ull << src);
    }
}

}  // namespace
