// vnbr.hip -- the neighbour table of a set of active voxels and the row gather through it on MI355X (gfx950): what a submanifold
// sparse convolution (SECOND, CenterPoint, PV-RCNN, sparse U-Nets) needs before its GEMM.  An extension: the reference stops at the
// voxelizer.
//
//   d3d_voxel_neighbors  coords[V,3] (+ batch[V]) -> table[V,K] int32: the row of the voxel at every kernel offset, -1 = none
//   d3d_neighbor_gather  feat[V,C], table[R,K]    -> out[R,K,C]: the neighbours' rows side by side, a zero row where there is none
//   d3d_voxel_corners    coords[V,3], positions[P,3] -> table[P,J] int32 and weights[P,J]: the rows of the 8 voxels around every
//                        fractional position (or of the nearest one) and their trilinear weights, for vinterp.hip
//
// The table: three launches, every dependency a kernel boundary (no workgroup waits on another inside a launch).
//   k_vn_bounds  min / max of every axis and of the batch value: integer atomicMax, one per wavefront and quantity (vkey.hpp: shared
//                with vstride.hip, as the table is)
//   k_vn_insert  key = mixed radix over the measured spans (one 64-bit number per voxel, below 2^62) into the open-addressing table
//                of vkey.hpp, {key, row} in one 16-byte slot: who claims the key stores its row; an equal key already there is a
//                duplicate
//   k_vn_lookup  one lane per (voxel, column), the column fastest: a wavefront's stores to `table` are contiguous.  A neighbour
//                outside the measured box is absent without a probe, so a shifted key never aliases another row; the centre is
//                the row itself, without a probe
//   k_vc_lookup  (d3d_voxel_corners: after the same two launches) one lane per (point, corner), the corner fastest
// Which slot a key lands in depends on the order the lanes arrive in; what a lookup finds does not: the same table on every run.
// The relation is symmetric -- table[v,k] == u <=> table[u,K-1-k] == v -- so the gradient of "gather my neighbours' rows" is the
// gather through the mirrored columns: forward and backward are gathers, nothing is scattered, no float atomics.
#include <algorithm>
#include "vkey.hpp"
#include "vrow.hpp"

namespace {

constexpr int64_t kNbrLookupBlocks = 1ll << 24;
constexpr int64_t kNbrGatherBlocks = 1ll << 30;
constexpr int64_t kVcLookupBlocks = 2048;     // grid-stride: a wavefront adds its found entries to counts[0] ONCE, 8 k atomics in all

struct alignas(16) NbrSlot {
    unsigned long long key;
    int32_t row, pad;
};

struct NbrShape {
    int32_t k[3], d[3];
};

struct NbrWs {
    unsigned long long *bounds;      // [4][2]: max(u), max(~u) of x, y, z, batch (u = value ^ sign); zero = nothing seen
    NbrSlot *slots;
    int log2cap;
};
// the one layout: carved here for d3d_voxel_neighbors, and on a null base for the size query
NbrWs nbr_carve(WsCarver &w, int64_t v)
{
    NbrWs r;
    r.log2cap = nbr_log2cap((unsigned long long)v);
    r.bounds = w.take<unsigned long long>(8);
    r.slots = w.take<NbrSlot>((size_t)1 << r.log2cap);
    return r;
}

// the measured box: lo[a] the smallest value of axis a (as uint64 bits of the int64), span[a] = max - min + 1; axis 3 = batch
struct NbrFrame {
    unsigned long long lo[4], span[4];
    bool overflow;
    // position inside the box; the difference of two int64 fits uint64
    __device__ unsigned long long rel(int a, int64_t x) const { return (unsigned long long)x - lo[a]; }
    __device__ unsigned long long key(const unsigned long long r[4]) const { return ((r[3] * span[0] + r[0]) * span[1] + r[1]) * span[2] + r[2]; }
};
__device__ __forceinline__ NbrFrame nbr_frame(const unsigned long long *__restrict__ bounds, bool has_batch)
{
    NbrFrame f;
    unsigned long long prod = 1;
    f.overflow = false;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        if (a == 3 && !has_batch) {
            f.lo[a] = 0;
            f.span[a] = 1;
            continue;
        }
        unsigned long long lo, hi;
        nbr_axis(bounds, a, lo, hi);
        f.lo[a] = lo ^ kNbrSign;
        f.span[a] = hi - lo + 1;                                        // 0: the whole int64 range
        if (f.span[a] == 0 || f.span[a] > kNbrSpanLimit / prod) f.overflow = true;
        else prod *= f.span[a];
    }
    return f;
}

__global__ __launch_bounds__(kNbrThreads) void k_vn_insert(const int64_t *__restrict__ coords, const int64_t *__restrict__ batch, int64_t v,
                                                           const unsigned long long *__restrict__ bounds, NbrSlot *__restrict__ slots,
                                                           int log2cap, int64_t *__restrict__ counts)
{
    const NbrFrame f = nbr_frame(bounds, batch != nullptr);
    if (f.overflow) {                                                   // (the same verdict in every lane of the launch)
        if (blockIdx.x == 0 && threadIdx.x == 0) counts[2] = 1;
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * kNbrThreads + threadIdx.x;
    bool dup = false;
    if (i < v) {
        const unsigned long long r[4] = {f.rel(0, coords[i * 3]), f.rel(1, coords[i * 3 + 1]), f.rel(2, coords[i * 3 + 2]),
                                         batch ? f.rel(3, batch[i]) : 0ull};
        bool fresh = false;
        const int64_t h = nbr_claim(slots, f.key(r), log2cap, fresh);
        if (h >= 0 && fresh) slots[h].row = (int32_t)i;
        dup = h >= 0 && !fresh;                                         // (the key was there: the same batch value and coordinate)
    }
    const unsigned long long b = __ballot(dup);
    if (b && (threadIdx.x & (kWave - 1)) == 0) atomicAdd((unsigned long long *)&counts[1], (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(kNbrThreads) void k_vn_lookup(const int64_t *__restrict__ coords, const int64_t *__restrict__ batch, int64_t v,
                                                           NbrShape s, const unsigned long long *__restrict__ bounds,
                                                           const NbrSlot *__restrict__ slots, int log2cap, int32_t *__restrict__ table,
                                                           int64_t *__restrict__ counts)
{
    const NbrFrame f = nbr_frame(bounds, batch != nullptr);
    if (f.overflow) return;
    const uint32_t K = (uint32_t)(s.k[0] * s.k[1] * s.k[2]), centre = (K - 1) / 2;
    const int64_t n = v * (int64_t)K;
    unsigned long long found = 0;
    // (every lane of a workgroup makes the same number of trips: the sum below runs on whole wavefronts)
    for (int64_t base = (int64_t)blockIdx.x * kNbrThreads; base < n; base += (int64_t)gridDim.x * kNbrThreads) {
        const int64_t v0 = base / K;                                    // one 64-bit division per workgroup and trip
        const uint32_t q = (uint32_t)(base - v0 * K) + threadIdx.x;
        const int64_t vi = v0 + q / K;
        const uint32_t k = q % K;
        if (vi >= v) continue;
        int32_t e = -1;
        if (k == centre) e = (int32_t)vi;
        else {
            int32_t ik[3];
            nbr_column(k, s.k, ik);
            unsigned long long r[4];
            bool inside = true;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                // a position is below 2^62 and a step below 2^34: the sum stays inside int64
                const int64_t p = (int64_t)f.rel(a, coords[vi * 3 + a]) + (int64_t)(ik[a] - (s.k[a] - 1) / 2) * s.d[a];
                inside &= p >= 0 && (unsigned long long)p < f.span[a];
                r[a] = (unsigned long long)p;
            }
            if (inside) {
                r[3] = batch ? f.rel(3, batch[vi]) : 0ull;
                NbrSlot sl;
                if (nbr_find(slots, f.key(r), log2cap, sl) >= 0) e = sl.row;
            }
        }
        table[vi * K + k] = e;
        found += e >= 0;
    }
    const unsigned long long total = wave_sum_u64(found);
    if (total && (threadIdx.x & (kWave - 1)) == 0) atomicAdd((unsigned long long *)&counts[0], total);
}

// ---------------------------------------------------------------- the corner table
// d3d_voxel_corners: the same bounds and insert launches, then one lane per (point, corner), the corner fastest: the J = 8 lanes of
// a point are neighbours in one wavefront (256 and 64 are multiples of 8), its stores to `table` and `weights` contiguous.  Per axis
// b = floor(x), f = x - b in the positions' type T; corner j = dx * 4 + dy * 2 + dz is the voxel at b + (dx, dy, dz), its weight
// (wx * wy) * wz with wa = f_a where the corner's bit is set, else 1 - f_a.  J = 1: the one corner floor(x + 0.5), weight 1.  A
// position that is not finite or not in [-2^62, 2^62) has no corners; a corner outside the measured box (its batch value included)
// is absent without a probe.  normalize: the point's lanes exchange their weights and every one folds s = 0 + w_j0 + w_j1 + ... over
// the present corners in ascending j itself.
template <typename T, int J>
__global__ __launch_bounds__(kNbrThreads) void k_vc_lookup(const T *__restrict__ pos, const int64_t *__restrict__ pos_batch, int64_t k,
                                                           bool has_batch, int32_t normalize, const unsigned long long *__restrict__ bounds,
                                                           const NbrSlot *__restrict__ slots, int log2cap, int32_t *__restrict__ table,
                                                           T *__restrict__ weights, int64_t *__restrict__ counts)
{
    const NbrFrame f = nbr_frame(bounds, has_batch);
    if (f.overflow) return;
    const int64_t n = k * J;
    const T limit = (T)4611686018427387904.0;                          // 2^62
    unsigned long long found = 0;
    // (every lane of a workgroup makes the same number of trips, and no lane leaves a trip early: the shuffles and the sum below run
    // on whole wavefronts)
    for (int64_t base = (int64_t)blockIdx.x * kNbrThreads; base < n; base += (int64_t)gridDim.x * kNbrThreads) {
        const int64_t idx = base + threadIdx.x, p = idx / J;
        const int j = (int)(idx % J);
        const bool live = idx < n;
        int32_t e = -1;
        T w = 0;
        if (live) {
            unsigned long long r[4];
            bool inside = true;
            w = 1;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const T x = pos[p * 3 + a];
                inside &= x >= -limit && x < limit;                     // (false for a NaN)
                const int bit = J == 8 ? (j >> (2 - a)) & 1 : 0;
                const T b = J == 8 ? floor(x) : floor(x + (T)0.5);
                if constexpr (J == 8) {
                    const T fr = x - b, wa = bit ? fr : (T)1 - fr;
                    w = a == 0 ? wa : w * wa;
                }
                // |b| <= 2^62 here: the conversion is exact and the corner stays inside int64
                const int64_t cell = (inside ? (int64_t)b : 0) + bit, lo = (int64_t)f.lo[a];
                inside &= cell >= lo && (unsigned long long)cell - (unsigned long long)lo < f.span[a];
                r[a] = (unsigned long long)cell - (unsigned long long)lo;
            }
            r[3] = 0;
            if (has_batch) {
                const int64_t pb = pos_batch[p], lo = (int64_t)f.lo[3];
                inside &= pb >= lo && (unsigned long long)pb - (unsigned long long)lo < f.span[3];
                r[3] = (unsigned long long)pb - (unsigned long long)lo;
            }
            if (inside) {
                NbrSlot sl;
                if (nbr_find(slots, f.key(r), log2cap, sl) >= 0) e = sl.row;
            }
            if (e < 0) w = 0;
        }
        if (J == 8 && normalize) {
            T s = 0;
#pragma unroll
            for (int q = 0; q < J; q++) {
                const T wq = __shfl(w, q, J);
                const int32_t eq = __shfl(e, q, J);
                if (eq >= 0) s = s + wq;
            }
            w = (e >= 0 && s != (T)0) ? w / s : (T)0;
        }
        if (live) {
            table[idx] = e;
            weights[idx] = w;
        }
        found += e >= 0;
    }
    const unsigned long long total = wave_sum_u64(found);
    if (total && (threadIdx.x & (kWave - 1)) == 0) atomicAdd((unsigned long long *)&counts[0], total);
}

// ---------------------------------------------------------------- the gather
// One lane group (1 << group_log2 lanes) per output row j = r * K + k, lane g of it on the VEC channels from g * VEC, then from
// (g + group) * VEC, ...  The source row: feat[e] (feat_cols == 1) or feat[e, k] (feat_cols == K: feat is [V, K, C]), with
// e = table[r, mirrored ? K - 1 - k : k]; a zero row for e == -1.
template <typename T, int VEC>
__global__ __launch_bounds__(kNbrThreads) void k_nbr_gather(const T *__restrict__ feat, const int32_t *__restrict__ table, int64_t rows,
                                                            int32_t K, int32_t c, int32_t feat_cols, int32_t mirrored, int group_log2,
                                                            int64_t nblk, T *__restrict__ out)
{
    typedef RowPack<T, VEC> P;
    const int per_block = kNbrThreads >> group_log2, g = (int)(threadIdx.x & ((1u << group_log2) - 1)), step = VEC << group_log2;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t j0 = blk * per_block, r0 = j0 / K;               // one 64-bit division per workgroup and trip
        const uint32_t q = (uint32_t)(j0 - r0 * K) + (threadIdx.x >> group_log2);
        const int64_t j = j0 + (threadIdx.x >> group_log2), r = r0 + q / (uint32_t)K;
        const int32_t k = (int32_t)(q % (uint32_t)K);
        if (j >= rows) continue;
        const int32_t e = table[r * K + (mirrored ? K - 1 - k : k)];
        const T *src = e >= 0 ? feat + ((int64_t)e * feat_cols + (feat_cols > 1 ? k : 0)) * c : nullptr;
        T *dst = out + j * c;
        for (int c0 = g * VEC; c0 < c; c0 += step) {
            P o;
#pragma unroll
            for (int x = 0; x < VEC; x++) o.v[x] = 0;
            if (src) o = *(const P *)(src + c0);
            *(P *)(dst + c0) = o;
        }
    }
}

bool nbr_shape_ok(const NbrShape &s)
{
    for (int a = 0; a < 3; a++)
        if (s.k[a] < 1 || s.k[a] > 7 || s.k[a] % 2 == 0 || s.d[a] < 1) return false;
    return true;
}

// what both tables begin with: counts zeroed and, for v > 0, the table of the voxels' keys -- the bounds and the insert launch
int nbr_build(const int64_t *coords, const int64_t *batch, int64_t v, const NbrWs &ws, int64_t *counts, hipStream_t st)
{
    D3D_HIP_CHECK(hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st));
    if (v == 0) return D3D_OK;
    D3D_HIP_CHECK(hipMemsetAsync(ws.bounds, 0, 8 * sizeof(unsigned long long), st));
    D3D_HIP_CHECK(hipMemsetAsync(ws.slots, 0xff, sizeof(NbrSlot) << ws.log2cap, st));
    const int64_t vb = d3d_divup(v, kNbrThreads);
    D3D_LAUNCH("k_vn_bounds", k_vn_bounds, dim3((unsigned)std::min<int64_t>(vb, kNbrBoundsBlocks)), dim3(kNbrThreads), 0, st, coords, batch, v,
               ws.bounds);
    D3D_LAUNCH("k_vn_insert", k_vn_insert, dim3((unsigned)vb), dim3(kNbrThreads), 0, st, coords, batch, v, ws.bounds, ws.slots, ws.log2cap,
               counts);
    return D3D_OK;
}

}  // namespace

extern "C" size_t d3d_voxel_neighbors_workspace_bytes(int64_t v)
{
    WsCarver w(nullptr, 0);
    nbr_carve(w, std::min(std::max<int64_t>(v, 0), kRowMax));
    return w.off;
}

extern "C" int d3d_voxel_neighbors(const int64_t *coords, const int64_t *batch, int64_t v, int32_t kx, int32_t ky, int32_t kz, int32_t dx,
                                   int32_t dy, int32_t dz, int32_t *table, int64_t *counts, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const NbrShape s{{kx, ky, kz}, {dx, dy, dz}};
    if (v < 0 || !counts || !nbr_shape_ok(s) || (v > 0 && (!coords || !table))) return D3D_ERR_BAD_ARG;
    if (v > kRowMax) return D3D_ERR_UNSUPPORTED;
    WsCarver w(workspace, workspace_bytes);
    const NbrWs ws = nbr_carve(w, v);
    if (v > 0 && (!workspace || !w.ok())) return D3D_ERR_WORKSPACE;
    if (const int rc = nbr_build(coords, batch, v, ws, counts, st); rc != D3D_OK || v == 0) return rc;
    const int64_t n = v * (int64_t)(kx * ky * kz);
    D3D_LAUNCH("k_vn_lookup", k_vn_lookup, dim3((unsigned)std::min(d3d_divup(n, kNbrThreads), kNbrLookupBlocks)), dim3(kNbrThreads), 0, st,
               coords, batch, v, s, ws.bounds, ws.slots, ws.log2cap, table, counts);
    return D3D_OK;
}

extern "C" size_t d3d_voxel_corners_workspace_bytes(int64_t v) { return d3d_voxel_neighbors_workspace_bytes(v); }

extern "C" int d3d_voxel_corners(const int64_t *coords, const int64_t *batch, int64_t v, const void *positions, const int64_t *position_batch,
                                 int64_t k, int32_t dtype, int32_t corners, int32_t normalize, int32_t *table, void *weights, int64_t *counts,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (v < 0 || k < 0 || !counts || (corners != 1 && corners != 8) || (v > 0 && !coords) || (k > 0 && (!positions || !table || !weights)) ||
        (v > 0 && k > 0 && (batch != nullptr) != (position_batch != nullptr)))
        return D3D_ERR_BAD_ARG;
    if ((dtype != D3D_F32 && dtype != D3D_F64) || v > kRowMax || k > kRowMax / corners) return D3D_ERR_UNSUPPORTED;
    WsCarver w(workspace, workspace_bytes);
    const NbrWs ws = nbr_carve(w, v);
    if (v > 0 && (!workspace || !w.ok())) return D3D_ERR_WORKSPACE;
    if (const int rc = nbr_build(coords, batch, v, ws, counts, st); rc != D3D_OK) return rc;
    const int64_t n = k * corners;
    if (v == 0) {                                                       // no voxel, no corner: -1 and weight 0 everywhere
        if (n > 0) {
            D3D_HIP_CHECK(hipMemsetAsync(table, 0xff, (size_t)n * sizeof(int32_t), st));
            D3D_HIP_CHECK(hipMemsetAsync(weights, 0, (size_t)n * (dtype == D3D_F64 ? 8 : 4), st));
        }
        return D3D_OK;
    }
    if (n == 0) return D3D_OK;
    return dispatch_dtype<D3D_F32, D3D_F64>(dtype, [&](auto p) {
        typedef typename decltype(p)::T T;
        return dispatch_int<1, 8>(corners, [&](auto jj) {
            D3D_LAUNCH("k_vc_lookup", (k_vc_lookup<T, decltype(jj)::value>), dim3((unsigned)std::min(d3d_divup(n, kNbrThreads), kVcLookupBlocks)),
                       dim3(kNbrThreads), 0, st, (const T *)positions, position_batch, k, batch != nullptr, normalize, ws.bounds, ws.slots,
                       ws.log2cap, table, (T *)weights, counts);
            return D3D_OK;
        });
    });
}

extern "C" int d3d_neighbor_gather(const void *feat, int64_t v, int32_t c, int32_t dtype, int32_t feat_cols, const int32_t *table, int64_t r,
                                   int32_t k, int32_t mirrored, void *out, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (v < 0 || r < 0 || c < 1 || k < 1 || (feat_cols != 1 && feat_cols != k)) return D3D_ERR_BAD_ARG;
    if ((dtype != D3D_F32 && dtype != D3D_F64) || v > kRowMax || k > 343 || r > kRowMax) return D3D_ERR_UNSUPPORTED;
    if (r == 0) return D3D_OK;
    if (!table || !out || (v > 0 && !feat)) return D3D_ERR_BAD_ARG;
    return row_dispatch<D3D_F32, D3D_F64>(dtype, c, row_aligned16(feat) && row_aligned16(out), [&](auto p, auto vec, int gl) {
        typedef typename decltype(p)::T T;
        const int64_t rows = r * k, nblk = d3d_divup(rows, kNbrThreads >> gl);
        D3D_LAUNCH("k_nbr_gather", (k_nbr_gather<T, decltype(vec)::value>), dim3((unsigned)std::min(nblk, kNbrGatherBlocks)), dim3(kNbrThreads), 0,
                   st, (const T *)feat, table, rows, k, c, feat_cols, mirrored, gl, nblk, (T *)out);
        return D3D_OK;
    });
}
