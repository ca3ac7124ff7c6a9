// vkey.hpp -- what vnbr.hip and vstride.hip share: the measurement of the coordinate box (one 64-bit mixed-radix key per voxel is
// formed over its spans) and its reading, the decoding of a kernel column, and the open-addressing table of such keys: its
// capacity, its hash, the claim of a slot and the search for one.  A slot is 16 bytes, `key` first; what its second word means
// is its owner's business (NbrSlot, ScSlot).
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

// axis a of the measured box (3: the batch value) from the words of k_vn_bounds: its smallest and largest value as order-keeping
// uint64 (value ^ kNbrSign); hi - lo = max - min fits uint64
__device__ __forceinline__ void nbr_axis(const unsigned long long *__restrict__ bounds, int a, unsigned long long &lo, unsigned long long &hi)
{
    hi = bounds[2 * a], lo = ~bounds[2 * a + 1];
}

// column k of a kernel of ks[0] x ks[1] x ks[2], the last axis fastest -> its index per axis
__device__ __forceinline__ void nbr_column(uint32_t k, const int32_t (&ks)[3], int32_t (&ik)[3])
{
    const uint32_t kyz = (uint32_t)(ks[1] * ks[2]);
    ik[0] = (int32_t)(k / kyz), ik[1] = (int32_t)(k % kyz) / ks[2], ik[2] = (int32_t)(k % kyz) % ks[2];
}

// the table of n keys: a power of two >= 2 n slots, 64 at least -- it is never more than half full, so a probe chain ends
__host__ __device__ inline int nbr_log2cap(unsigned long long n)
{
    int log2cap = 6;
    while ((1ull << log2cap) < 2 * n) log2cap++;
    return log2cap;
}

__device__ __forceinline__ unsigned long long nbr_hash(unsigned long long key, int log2cap) { return (key * kNbrMix) >> (64 - log2cap); }

// The slot of `key`, claimed by an atomicCAS on the slots' keys (all kNbrEmpty at first), linear probing from its hash; fresh: this
// call put the key there (exactly one of the calls with a key sees that).  Which slot it is depends on the order the lanes arrive
// in.  (-1 after the whole table: not reached while the table is at most half full)
template <class Slot>
__device__ __forceinline__ int64_t nbr_claim(Slot *slots, unsigned long long key, int log2cap, bool &fresh)
{
    const unsigned long long mask = (1ull << log2cap) - 1;
    unsigned long long h = nbr_hash(key, log2cap);
    for (unsigned long long t = 0; t <= mask; t++, h = (h + 1) & mask) {
        const unsigned long long old = atomicCAS(&slots[h].key, kNbrEmpty, key);
        if (old == kNbrEmpty || old == key) {
            fresh = old == kNbrEmpty;
            return (int64_t)h;
        }
    }
    return -1;
}

// The slot of a key that was claimed, -1 for one that was not: the probe ends at the key, at an empty slot or after the whole
// table.  sl: the slot as this one 16-byte load saw it (both words together).
template <class Slot>
__device__ __forceinline__ int64_t nbr_find(const Slot *slots, unsigned long long key, int log2cap, Slot &sl)
{
    const unsigned long long mask = (1ull << log2cap) - 1;
    unsigned long long h = nbr_hash(key, log2cap);
    for (unsigned long long t = 0; t <= mask; t++, h = (h + 1) & mask) {
        sl = slots[h];
        if (sl.key == key) return (int64_t)h;
        if (sl.key == kNbrEmpty) break;
    }
    return -1;
}

}  // namespace
