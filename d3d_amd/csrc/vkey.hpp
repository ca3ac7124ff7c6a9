// vkey.hpp -- what vnbr.hip and vstride.hip share: the measurement of the coordinate box (one 64-bit mixed-radix key per voxel is
// formed over its spans) and the hash of such a key.
#pragma once
#include "common.hpp"

namespace {

constexpr int kNbrThreads = 256;
constexpr int kNbrBoundsBlocks = 1024;                 // grid-stride: 8 atomics per wavefront, 32 k in all at most
constexpr unsigned long long kNbrEmpty = ~0ull;        // (keys stay below 2^62)
constexpr unsigned long long kNbrSpanLimit = 1ull << 62;
constexpr unsigned long long kNbrSign = 1ull << 63;    // x ^ sign: int64 -> uint64, order kept
constexpr unsigned long long kNbrMix = 0x9e3779b97f4a7c15ull;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long x)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const unsigned long long y = __shfl_xor(x, d, kWave);
        x = y > x ? y : x;
    }
    return x;
}

__global__ __launch_bounds__(kNbrThreads) void k_vn_bounds(const int64_t *__restrict__ coords, const int64_t *__restrict__ batch, int64_t v,
                                                           unsigned long long *__restrict__ bounds)
{
    unsigned long long m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * kNbrThreads + threadIdx.x; i < v; i += (int64_t)gridDim.x * kNbrThreads) {
#pragma unroll
        for (int a = 0; a < 4; a++) {
            if (a == 3 && !batch) continue;
            const unsigned long long u = (unsigned long long)(a < 3 ? coords[i * 3 + a] : batch[i]) ^ kNbrSign;
            m[2 * a] = u > m[2 * a] ? u : m[2 * a];
            m[2 * a + 1] = ~u > m[2 * a + 1] ? ~u : m[2 * a + 1];
        }
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const unsigned long long w = wave_max_u64(m[q]);
        if ((threadIdx.x & (kWave - 1)) == 0 && w) atomicMax(&bounds[q], w);
    }
}

__device__ __forceinline__ unsigned long long nbr_hash(unsigned long long key, int log2cap) { return (key * kNbrMix) >> (64 - log2cap); }

}  // namespace
