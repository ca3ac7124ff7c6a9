// pgrid.hip -- a uniform cell index of a cloud (PointGrid) and the two neighbour searches over it, on MI355X (gfx950): the
// grid-accelerated siblings of psample.hip's d3d_ball_query / d3d_knn_query.  They return the SAME BITS (tables, counts, dist2,
// padding, global rows) and read only the cells a centre can reach: a whole frame against itself (KPConv, PointNeXt, Point
// Transformer, Voxel R-CNN's voxel query, normals) instead of O(m n).  The rules stand in include/d3d_hip.h, the proofs that the
// walked cells are a superset of what the brute-force route would find in DESIGN.md 8j.  An extension: the reference has no
// point sampling.
//
//   d3d_point_grid_bounds   per segment min / max of the finite rows (fp64) and their number: integer atomics on order-keeping keys
//   d3d_point_grid_plan     PURE HOST: bounds -> per segment lo, h (cell_size doubled until the cells fit the cap), 1 / h, dims, base
//   d3d_point_grid_build    one lane per row: its cell; d3d_voxel_index's launches (rows grouped by cell, ascending row inside a
//                           cell); one lane per entry: the coordinates in cell order beside `order` (two coalesced streams per walk)
//   d3d_ball_query_grid     one wavefront per centre: the box of cells around it, (y, z) by (y, z) one contiguous run of `order`
//   d3d_knn_query_grid      one wavefront per centre: rings of cells around its own, until the k-th key is nearer than every
//                           unexplored cell
// The walk: the runs of a box (of a ring) are numbered; 64 of them at a time, each lane reads the two offsets of one (ONE round trip
// for 64 runs, and a ballot drops the empty ones); every run that holds rows is then walked by the whole wavefront 4 x 64 entries at
// a time, all four tiles loaded before the first is judged, as the siblings walk a segment.  q is pquery.hpp's, the held keys and
// their insertion too: the ball query keeps the nsample LOWEST rows inside (key = the row alone: cells do not come in row order),
// the kNN the k smallest (q, row).  No LDS, no atomics, no workspace, nothing waits on another wavefront.
#include "common.hpp"
#include "pquery.hpp"

#include <cmath>
#include <limits>

namespace {

constexpr int64_t kPgRowMax = 0x7fffffffll;
constexpr int kPgThreads = 256;
constexpr int kPgWaves = kPgThreads / kWave;
constexpr int kPgAhead = 4;                    // tiles of 64 entries in flight per wavefront
constexpr int kPgMaxSample = 1024;             // what d3d_ball_query takes: above it a bad argument, above D3D_KNN_MAX unsupported here
constexpr double kPgSlack = 0x1p-20;           // the relative slack of the ball box and of the kNN bound
constexpr double kPgOut = 0x1p-50;             // a box edge is moved outward by this much of itself: above its own rounding

bool pg_dtype_ok(int32_t dtype) { return dtype == D3D_F32 || dtype == D3D_F64; }

// ---------------------------------------------------------------- bounds
// a double as an unsigned integer that orders like it (-0.0 below +0.0); never 0 and never all ones for a finite value, so that 0
// is "nothing yet" of a maximum both of the key (the largest value) and of its complement (the smallest)
__device__ __forceinline__ unsigned long long pg_order_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double pg_order_value(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k ^ (1ull << 63)) : ~k));
}

// the segment of a ROW: point_offsets[b] <= i < point_offsets[b + 1] (ps_segment_of's search: the last b that starts at or below i
// is the one that holds it, empty segments in front of it start there as well)
__device__ __forceinline__ int64_t pg_row_segment(const int64_t *__restrict__ point_offsets, int64_t segments, int64_t i)
{
    return point_offsets ? ps_segment_of(point_offsets, segments, i) : 0;
}

// One lane per row.  slots[s * 6 + a] collects ~key(min) for a = 0 .. 2 and key(max) for a = 3 .. 5 as maxima of unsigned integers,
// finite[s] the number of finite rows.  A wavefront whose rows lie in one segment (all but the few on a boundary) reduces first and
// sends seven atomics; the result does not depend on any order: integer maxima and an integer sum.
template <typename T>
__global__ __launch_bounds__(kPgThreads) void k_pg_bounds(const T *__restrict__ points, int64_t n, int32_t stride,
                                                          const int64_t *__restrict__ point_offsets, int64_t segments,
                                                          unsigned long long *__restrict__ slots, unsigned long long *__restrict__ finite)
{
    const int64_t i = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long key[6] = {0, 0, 0, 0, 0, 0};
    bool ok = false;
    int64_t s = -1;
    if (i < n) {
        const T *p = points + i * stride;
        const T x = p[0], y = p[1], z = p[2];
        s = pg_row_segment(point_offsets, segments, i);
        if (ps_finite3(x, y, z)) {
            ok = true;
            key[3] = pg_order_key((double)x), key[4] = pg_order_key((double)y), key[5] = pg_order_key((double)z);
            key[0] = ~key[3], key[1] = ~key[4], key[2] = ~key[5];
        }
    }
    const unsigned long long has = __ballot(ok);
    if (has == 0) return;                      // (wave-uniform)
    const int src = __ffsll((long long)has) - 1;
    const int64_t s0 = (int64_t)wave_readlane((uint64_t)s, src);
    if (__ballot(ok && s != s0) == 0) {        // one segment: reduce, then the lane `src` alone
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int d = kWave / 2; d > 0; d >>= 1) {
                const unsigned long long o = __shfl_xor(key[a], d, kWave);
                if (o > key[a]) key[a] = o;
            }
        }
        if (lane == src) {
#pragma unroll
            for (int a = 0; a < 6; a++) atomicMax(&slots[s0 * 6 + a], key[a]);
            atomicAdd(&finite[s0], (unsigned long long)__popcll(has));
        }
    } else if (ok) {
#pragma unroll
        for (int a = 0; a < 6; a++) atomicMax(&slots[s * 6 + a], key[a]);
        atomicAdd(&finite[s], 1ull);
    }
}

// one lane per segment: the keys back to doubles, in place; a segment without a finite row: zeros
__global__ __launch_bounds__(kPgThreads) void k_pg_bounds_decode(unsigned long long *__restrict__ slots, const unsigned long long *__restrict__ finite,
                                                                 int64_t segments)
{
    const int64_t s = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
    if (s >= segments) return;
    const bool any = finite[s] > 0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        const unsigned long long k = slots[s * 6 + a];
        slots[s * 6 + a] = (unsigned long long)__double_as_longlong(any ? pg_order_value(a < 3 ? ~k : k) : 0.0);
    }
}

// ---------------------------------------------------------------- the cell of a coordinate
// clamp(floor(t * inv_h), 0, dim - 1) of t = fp64(x) - lo, clamped while still a double; a NaN gives 0.  Monotone in t.
__host__ __device__ inline int32_t pg_cell_rel(double t, double inv_h, int32_t dim)
{
    const double f = floor(t * inv_h);
    if (!(f > 0.0)) return 0;                  // (NaN as well)
    const double top = (double)(dim - 1);
    return (int32_t)(f < top ? f : top);
}

// one lane per row: NaN -> -1, an infinite coordinate -> the segment's overflow cell, else its cell
template <typename T>
__global__ __launch_bounds__(kPgThreads) void k_pg_mapping(const T *__restrict__ points, int64_t n, int32_t stride,
                                                           const int64_t *__restrict__ point_offsets, int64_t segments,
                                                           const D3DPointGridSegment *__restrict__ plan, int64_t *__restrict__ mapping)
{
    const int64_t i = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
    if (i >= n) return;
    const T *p = points + i * stride;
    const T x = p[0], y = p[1], z = p[2];
    const D3DPointGridSegment g = plan[pg_row_segment(point_offsets, segments, i)];
    int64_t id;
    if (x != x || y != y || z != z) {
        id = -1;
    } else if (!ps_finite3(x, y, z)) {
        id = g.base + (int64_t)g.dim[0] * g.dim[1] * g.dim[2];
    } else {
        const int64_t cx = pg_cell_rel((double)x - g.lo[0], g.inv_h, g.dim[0]), cy = pg_cell_rel((double)y - g.lo[1], g.inv_h, g.dim[1]),
                      cz = pg_cell_rel((double)z - g.lo[2], g.inv_h, g.dim[2]);
        id = g.base + (cz * g.dim[1] + cy) * g.dim[0] + cx;
    }
    mapping[i] = id;
}

// one lane per entry of `order`: its row's coordinates, in cell order
template <typename T>
__global__ __launch_bounds__(kPgThreads) void k_pg_pack(const T *__restrict__ points, int64_t n, int32_t stride, const int32_t *__restrict__ order,
                                                        const int64_t *__restrict__ counts, T *__restrict__ packed)
{
    const int64_t j = (int64_t)blockIdx.x * kPgThreads + threadIdx.x;
    if (j >= n || j >= counts[0]) return;
    const T *p = points + (int64_t)order[j] * stride;
    T *o = packed + j * 3;
    o[0] = p[0], o[1] = p[1], o[2] = p[2];
}

// ---------------------------------------------------------------- the walk
// entries [beg, end) of the cell-ordered streams, 4 x 64 at a time: tile(q, row) per tile of 64, in ascending entry; a lane past the
// end carries q = NaN (no candidate of either query) and row = all ones.  beg, end wave-uniform.
template <typename T, class Tile>
__device__ __forceinline__ void pg_walk(const T *__restrict__ packed, const int32_t *__restrict__ order, uint32_t beg, uint32_t end, int lane,
                                        T cx, T cy, T cz, Tile &&tile)
{
    for (uint32_t base = beg; base < end; base += kPgAhead * kWave) {
        T q[kPgAhead];
        uint32_t row[kPgAhead];
#pragma unroll
        for (int u = 0; u < kPgAhead; u++) {
            const uint32_t j = base + u * kWave + lane;
            q[u] = std::numeric_limits<T>::quiet_NaN(), row[u] = ~0u;
            if (j < end) {
                const T *p = packed + (int64_t)j * 3;
                q[u] = ps_q<T>(p[0], p[1], p[2], cx, cy, cz);
                row[u] = (uint32_t)order[j];
            }
        }
#pragma unroll
        for (int u = 0; u < kPgAhead; u++)
            if (base + u * kWave < end) tile(q[u], row[u]);                     // (wave-uniform)
    }
}

// runs 0 .. nruns - 1, run t = the cells a .. b (contiguous ids) that desc(t, a, b) names (false: none): 64 runs at a time every
// lane fetches the bounds of one, then the runs that hold rows are walked one after the other.  (entries are below 2^31: uint32)
template <typename T, class Desc, class Tile>
__device__ __forceinline__ void pg_runs(int64_t nruns, const int64_t *__restrict__ cell_offsets, const T *__restrict__ packed,
                                        const int32_t *__restrict__ order, int lane, T cx, T cy, T cz, Desc &&desc, Tile &&tile)
{
    for (int64_t t0 = 0; t0 < nruns; t0 += kWave) {
        const int64_t t = t0 + lane;
        uint32_t beg = 0, end = 0;
        int64_t a, b;
        if (t < nruns && desc(t, a, b)) beg = (uint32_t)cell_offsets[a], end = (uint32_t)cell_offsets[b + 1];
        unsigned long long vote = __ballot(end > beg);
        while (vote) {                         // (wave-uniform)
            const int src = __ffsll((long long)vote) - 1;
            vote &= vote - 1;
            pg_walk<T>(packed, order, wave_readlane(beg, src), wave_readlane(end, src), lane, cx, cy, cz, tile);
        }
    }
}

// t = q * d + r, with the 32-bit division wherever t allows it (always, short of 2^32 runs in one box)
__device__ __forceinline__ void pg_divmod(int64_t t, int64_t d, int64_t &q, int64_t &r)
{
    if (((uint64_t)t >> 32) == 0 && ((uint64_t)d >> 32) == 0) {
        const uint32_t q32 = (uint32_t)t / (uint32_t)d;
        q = q32, r = (uint32_t)t - q32 * (uint32_t)d;
    } else {
        q = t / d, r = t - q * d;
    }
}

// ---------------------------------------------------------------- ball query
// The box: per axis the cells of u - R .. u + R, u = fp64(x_c) - lo, R = r (1 + 2^-20), each edge moved outward by 2^-50 of itself
// (more than the rounding of u and of the sum): every row with q < r2 lies in it.  An edge that falls off the grid on
// the wrong side leaves an empty box.  The whole box is walked: cells do not come in row order, so the nsample lowest rows are known
// at the end only; they are kept sorted across the lanes, key = the row.
template <typename T>
__global__ __launch_bounds__(kPgThreads) void k_ball_query_grid(const T *__restrict__ centers, int64_t m, int32_t cstride,
                                                                const int64_t *__restrict__ center_offsets, int64_t segments,
                                                                const D3DPointGridSegment *__restrict__ plan, const int32_t *__restrict__ order,
                                                                const int64_t *__restrict__ cell_offsets, const T *__restrict__ packed, T r2,
                                                                double R, int32_t nsample, int32_t pad_first, int32_t *__restrict__ table,
                                                                int32_t *__restrict__ counts)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t c = (int64_t)blockIdx.x * kPgWaves + threadIdx.x / kWave;
    if (c >= m) return;
    const D3DPointGridSegment g = plan[center_offsets ? ps_segment_of(center_offsets, segments, c) : 0];
    const T *const q0 = centers + c * cstride;
    const T cx = q0[0], cy = q0[1], cz = q0[2];
    uint32_t held, tau;
    knn_clear(held), knn_clear(tau);
    int found = 0;
    if (ps_finite3(cx, cy, cz)) {              // (a centre that is not finite matches nothing)
        const double u[3] = {(double)cx - g.lo[0], (double)cy - g.lo[1], (double)cz - g.lo[2]};
        int32_t c0[3], c1[3];
        bool any = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            double e0 = u[a] - R, e1 = u[a] + R;
            e0 = e0 - fabs(e0) * kPgOut, e1 = e1 + fabs(e1) * kPgOut;
            if (e1 * g.inv_h < 0.0 || floor(e0 * g.inv_h) > (double)(g.dim[a] - 1)) any = false;
            c0[a] = pg_cell_rel(e0, g.inv_h, g.dim[a]), c1[a] = pg_cell_rel(e1, g.inv_h, g.dim[a]);
        }
        if (any) {
            const int64_t ny = c1[1] - c0[1] + 1, nz = c1[2] - c0[2] + 1;
            auto desc = [&](int64_t t, int64_t &a, int64_t &b) {
                int64_t zq, yr;
                pg_divmod(t, ny, zq, yr);
                a = g.base + ((c0[2] + zq) * g.dim[1] + (c0[1] + yr)) * g.dim[0] + c0[0];
                b = a + (c1[0] - c0[0]);
                return true;
            };
            auto tile = [&](T q, uint32_t row) {
                const bool in = q < r2;                                         // false for NaN
                found += __popcll(__ballot(in));
                knn_insert_tile(in ? row : ~0u, held, tau, lane, nsample);
            };
            pg_runs<T>(ny * nz, cell_offsets, packed, order, lane, cx, cy, cz, desc, tile);
        }
    }
    const int count = found < nsample ? found : nsample;
    const int32_t pad = (pad_first && count > 0) ? (int32_t)wave_readlane(held, 0) : -1;
    if (lane < nsample) table[c * nsample + lane] = lane < count ? (int32_t)held : pad;
    if (lane == 0) counts[c] = count;
}

// ---------------------------------------------------------------- k nearest rows
// Rings of cells around cc, the centre's own (clamped) cell: ring rho is the box [cc - rho, cc + rho] clamped to the grid, minus
// ring rho - 1's box: for every (y, z) of the box that was not inside before ONE run over the whole x range, for the others the two
// end cells.  After a ring, d = the least distance of the centre to a face of the box that is not on the grid's border, in
// coordinates relative to lo; every row not yet seen lies beyond such a face.  The walk ends once the k-th held key is nearer than
// that, STRICTLY (an unexplored row with equal q and a lower row number would win the tie), with the slack of DESIGN.md 8j.  When
// every face is on the border the grid is exhausted, and the overflow cell (rows with an infinite coordinate: q = +inf or NaN) is
// walked unless the k-th key is there with a finite q.
template <typename T>
__global__ __launch_bounds__(kPgThreads) void k_knn_query_grid(const T *__restrict__ centers, int64_t m, int32_t cstride,
                                                               const int64_t *__restrict__ center_offsets, int64_t segments,
                                                               const D3DPointGridSegment *__restrict__ plan, const int32_t *__restrict__ order,
                                                               const int64_t *__restrict__ cell_offsets, const T *__restrict__ packed, int32_t k,
                                                               int32_t *__restrict__ table, T *__restrict__ dist2)
{
    typedef typename KnnKeyOf<T>::type K;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t c = (int64_t)blockIdx.x * kPgWaves + threadIdx.x / kWave;
    if (c >= m) return;
    const D3DPointGridSegment g = plan[center_offsets ? ps_segment_of(center_offsets, segments, c) : 0];
    const T *const q0 = centers + c * cstride;
    const T cx = q0[0], cy = q0[1], cz = q0[2];
    K held, tau;
    knn_clear(held), knn_clear(tau);
    auto tile = [&](T q, uint32_t row) {
        K key;
        knn_clear(key);
        if (q == q) key = knn_make(q, row);                                     // (a NaN q: no candidate)
        knn_insert_tile(key, held, tau, lane, k);
    };
    if (cx == cx && cy == cy && cz == cz) {    // (a NaN centre has no candidate)
        const double u[3] = {(double)cx - g.lo[0], (double)cy - g.lo[1], (double)cz - g.lo[2]};
        const int64_t dim[3] = {g.dim[0], g.dim[1], g.dim[2]};
        const int64_t cc[3] = {pg_cell_rel(u[0], g.inv_h, g.dim[0]), pg_cell_rel(u[1], g.inv_h, g.dim[1]), pg_cell_rel(u[2], g.inv_h, g.dim[2])};
        const double least = 4.0 * (double)std::numeric_limits<T>::min();      // below it a term of q may have been flushed
        bool overflow = true;
        for (int64_t rho = 0;; rho++) {
            int64_t b0[3], b1[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                b0[a] = cc[a] - rho > 0 ? cc[a] - rho : 0;
                b1[a] = cc[a] + rho < dim[a] - 1 ? cc[a] + rho : dim[a] - 1;
            }
            const int64_t ny = b1[1] - b0[1] + 1, nz = b1[2] - b0[2] + 1;
            auto desc = [&](int64_t t, int64_t &a, int64_t &b) {
                int64_t zq, yr;
                pg_divmod(t >> 1, ny, zq, yr);
                const int64_t y = b0[1] + yr, z = b0[2] + zq, line = g.base + (z * dim[1] + y) * dim[0];
                const bool inner = y > cc[1] - rho && y < cc[1] + rho && z > cc[2] - rho && z < cc[2] + rho;
                if (!inner) {                  // a new (y, z): the whole x range, once
                    a = line + b0[0], b = line + b1[0];
                    return (t & 1) == 0;
                }
                const int64_t x = (t & 1) ? cc[0] + rho : cc[0] - rho;          // the two end cells, where they are on the grid
                a = b = line + x;
                return x >= 0 && x < dim[0] && (rho > 0 || (t & 1) == 0);
            };
            pg_runs<T>(2 * ny * nz, cell_offsets, packed, order, lane, cx, cy, cz, desc, tile);
            double d = std::numeric_limits<double>::infinity();
            bool open = false;                 // a face that is not on the border
#pragma unroll
            for (int a = 0; a < 3; a++) {
                if (cc[a] - rho > 0) {
                    const double gap = u[a] - (double)(cc[a] - rho) * g.h;
                    open = true;
                    if (gap < d) d = gap;
                }
                if (cc[a] + rho < dim[a] - 1) {
                    const double gap = (double)(cc[a] + rho + 1) * g.h - u[a];
                    open = true;
                    if (gap < d) d = gap;
                }
            }
            if (!open) break;                  // the grid is exhausted
            const double dd = d * (1.0 - kPgSlack) - kPgSlack * g.h;
            if (dd > 0.0 && !knn_none(tau)) {
                const double bound = dd * dd * (1.0 - kPgSlack);
                if ((double)knn_dist(tau, (T)0) < bound && bound >= least) {
                    overflow = false;
                    break;
                }
            }
        }
        if (overflow && (knn_none(tau) || !(knn_dist(tau, (T)0) < std::numeric_limits<T>::infinity()))) {
            const int64_t cell = g.base + dim[0] * dim[1] * dim[2];
            const uint32_t beg = (uint32_t)cell_offsets[cell], end = (uint32_t)cell_offsets[cell + 1];
            pg_walk<T>(packed, order, beg, end, lane, cx, cy, cz, tile);
        }
    }
    if (lane < k) {
        const bool none = knn_none(held);
        table[c * k + lane] = none ? -1 : (int32_t)knn_row(held);
        if (dist2) dist2[c * k + lane] = none ? std::numeric_limits<T>::infinity() : knn_dist(held, (T)0);
    }
}

// what both queries refuse before they look at their own arguments: D3D_OK to go on
int pg_query_check(int64_t n, int64_t m, int64_t segments, int32_t center_stride, int32_t dtype, const int64_t *center_offsets)
{
    if (n < 0 || m < 0 || segments < 0 || center_stride < 3) return D3D_ERR_BAD_ARG;
    if (center_offsets && segments < 1 && m > 0) return D3D_ERR_BAD_ARG;
    if (!pg_dtype_ok(dtype) || n > kPgRowMax || m > kPgRowMax || segments > kPgRowMax) return D3D_ERR_UNSUPPORTED;
    return D3D_OK;
}

}  // namespace

extern "C" int d3d_point_grid_bounds(const void *points, int64_t n, int32_t row_stride, int32_t dtype, const int64_t *point_offsets,
                                     int64_t segments, double *bounds, int64_t *finite_rows, void *stream)
{
    if (n < 0 || segments < 0 || row_stride < 3) return D3D_ERR_BAD_ARG;
    if (point_offsets && segments < 1 && n > 0) return D3D_ERR_BAD_ARG;
    if (!pg_dtype_ok(dtype) || n > kPgRowMax || segments > kPgRowMax) return D3D_ERR_UNSUPPORTED;
    const int64_t s = point_offsets ? segments : 1;
    if (s == 0) return D3D_OK;
    if (!bounds || !finite_rows || (n > 0 && !points)) return D3D_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *const slots = (unsigned long long *)bounds, *const fin = (unsigned long long *)finite_rows;
    D3D_HIP_CHECK(hipMemsetAsync(slots, 0, (size_t)s * 6 * sizeof(double), st));
    D3D_HIP_CHECK(hipMemsetAsync(fin, 0, (size_t)s * sizeof(int64_t), st));
    if (n > 0) {
        const dim3 grid((unsigned)d3d_divup(n, kPgThreads));
        if (dtype == D3D_F64) {
            D3D_LAUNCH("k_pg_bounds<f64>", k_pg_bounds<double>, grid, dim3(kPgThreads), 0, st, (const double *)points, n, row_stride, point_offsets,
                       s, slots, fin);
        } else {
            D3D_LAUNCH("k_pg_bounds<f32>", k_pg_bounds<float>, grid, dim3(kPgThreads), 0, st, (const float *)points, n, row_stride, point_offsets,
                       s, slots, fin);
        }
    }
    D3D_LAUNCH("k_pg_bounds_decode", k_pg_bounds_decode, dim3((unsigned)d3d_divup(s, kPgThreads)), dim3(kPgThreads), 0, st, slots, fin, s);
    return D3D_OK;
}

extern "C" int d3d_point_grid_plan(const double *bounds, const int64_t *finite_rows, int64_t segments, double cell_size,
                                   double max_cells_per_point, D3DPointGridSegment *plan, int64_t *total_cells)
{
    if (segments < 0 || !total_cells || (segments > 0 && (!bounds || !finite_rows || !plan))) return D3D_ERR_BAD_ARG;
    if (!(cell_size > 0) || !std::isfinite(cell_size) || !(max_cells_per_point > 0) || !std::isfinite(max_cells_per_point)) return D3D_ERR_BAD_ARG;
    if (segments > kPgRowMax) return D3D_ERR_UNSUPPORTED;
    for (int64_t s = 0; s < segments; s++) {
        if (finite_rows[s] < 0) return D3D_ERR_BAD_ARG;
        for (int a = 0; a < 3; a++)
            if (finite_rows[s] > 0 && !(std::isfinite(bounds[s * 6 + a]) && std::isfinite(bounds[s * 6 + 3 + a]) && bounds[s * 6 + a] <= bounds[s * 6 + 3 + a]))
                return D3D_ERR_BAD_ARG;
    }
    int64_t base = 0;
    for (int64_t s = 0; s < segments; s++) {
        D3DPointGridSegment &g = plan[s];
        const bool any = finite_rows[s] > 0;
        double ext[3];
        for (int a = 0; a < 3; a++) {
            g.lo[a] = any ? bounds[s * 6 + a] : 0.0;
            ext[a] = any ? bounds[s * 6 + 3 + a] - bounds[s * 6 + a] : 0.0;
            if (!std::isfinite(ext[a])) return D3D_ERR_UNSUPPORTED;             // (fp64 rows at both ends of the range)
        }
        const double cap = std::fmax(64.0, std::ceil(max_cells_per_point * (double)finite_rows[s]));
        double h = cell_size;
        // the quotients are compared as doubles, before any conversion to an integer: they may be 1e300
        while (!((std::floor(ext[0] / h) + 1.0) * (std::floor(ext[1] / h) + 1.0) * (std::floor(ext[2] / h) + 1.0) <= cap)) {
            h = h * 2.0;
            if (!std::isfinite(h)) return D3D_ERR_UNSUPPORTED;
        }
        g.h = h, g.inv_h = 1.0 / h;
        int64_t cells = 1;
        for (int a = 0; a < 3; a++) {
            const double dim = std::floor(ext[a] * g.inv_h) + 1.0;             // (<= cap + a rounding: far below 2^62)
            if (!(dim <= (double)kPgRowMax)) return D3D_ERR_UNSUPPORTED;
            g.dim[a] = (int32_t)dim;
            cells *= (int64_t)dim;
            if (cells > kPgRowMax) return D3D_ERR_UNSUPPORTED;
        }
        g.pad_ = 0;
        g.base = base;
        base += cells + 1;                     // (and the overflow cell)
        if (base > kPgRowMax) return D3D_ERR_UNSUPPORTED;
    }
    *total_cells = base;
    return D3D_OK;
}

extern "C" size_t d3d_point_grid_workspace_bytes(int64_t n, int64_t total_cells) { return d3d_voxel_index_workspace_bytes(n, total_cells); }

extern "C" int d3d_point_grid_build(const void *points, int64_t n, int32_t row_stride, int32_t dtype, const int64_t *point_offsets,
                                    int64_t segments, const D3DPointGridSegment *plan, int64_t total_cells, int64_t *mapping, int32_t *order,
                                    int64_t *offsets, int64_t *counts, void *packed, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || segments < 0 || row_stride < 3 || total_cells < 1) return D3D_ERR_BAD_ARG;
    if (point_offsets && segments < 1) return D3D_ERR_BAD_ARG;
    if (!pg_dtype_ok(dtype) || n > kPgRowMax || segments > kPgRowMax || total_cells > kPgRowMax) return D3D_ERR_UNSUPPORTED;
    if (!plan || !offsets || !counts || (n > 0 && (!points || !mapping || !order || !packed))) return D3D_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < d3d_voxel_index_workspace_bytes(n, total_cells)) return D3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d3d_divup(n, kPgThreads));
    if (n > 0) {
        if (dtype == D3D_F64) {
            D3D_LAUNCH("k_pg_mapping<f64>", k_pg_mapping<double>, grid, dim3(kPgThreads), 0, st, (const double *)points, n, row_stride,
                       point_offsets, segments, plan, mapping);
        } else {
            D3D_LAUNCH("k_pg_mapping<f32>", k_pg_mapping<float>, grid, dim3(kPgThreads), 0, st, (const float *)points, n, row_stride,
                       point_offsets, segments, plan, mapping);
        }
    }
    if (const int rc = d3d_voxel_index(mapping, n, total_cells, order, offsets, counts, workspace, workspace_bytes, stream); rc != D3D_OK) return rc;
    if (n > 0) {
        if (dtype == D3D_F64) {
            D3D_LAUNCH("k_pg_pack<f64>", k_pg_pack<double>, grid, dim3(kPgThreads), 0, st, (const double *)points, n, row_stride, order, counts,
                       (double *)packed);
        } else {
            D3D_LAUNCH("k_pg_pack<f32>", k_pg_pack<float>, grid, dim3(kPgThreads), 0, st, (const float *)points, n, row_stride, order, counts,
                       (float *)packed);
        }
    }
    return D3D_OK;
}

extern "C" int d3d_ball_query_grid(const void *centers, int64_t m, int32_t center_stride, int32_t dtype, const int64_t *center_offsets,
                                   int64_t segments, const D3DPointGridSegment *plan, const int32_t *order, const int64_t *cell_offsets,
                                   const void *packed, int64_t n, double radius, int32_t nsample, int32_t pad_first, int32_t *table,
                                   int32_t *counts, void *stream)
{
    if (nsample < 1 || nsample > kPgMaxSample || !(radius > 0) || !std::isfinite(radius)) return D3D_ERR_BAD_ARG;
    if (const int rc = pg_query_check(n, m, segments, center_stride, dtype, center_offsets); rc != D3D_OK) return rc;
    if (nsample > D3D_KNN_MAX) return D3D_ERR_UNSUPPORTED;                      // (the held rows: one per lane.  d3d_ball_query takes it)
    if (m == 0) return D3D_OK;
    if (!centers || !table || !counts || !plan || !cell_offsets || (n > 0 && (!order || !packed))) return D3D_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d3d_divup(m, kPgWaves));
    if (dtype == D3D_F64) {
        const double r = radius;
        D3D_LAUNCH("k_ball_query_grid<f64>", k_ball_query_grid<double>, grid, dim3(kPgThreads), 0, st, (const double *)centers, m, center_stride,
                   center_offsets, segments, plan, order, cell_offsets, (const double *)packed, r * r, r * (1.0 + kPgSlack), nsample, pad_first,
                   table, counts);
    } else {
        const float r = (float)radius;
        D3D_LAUNCH("k_ball_query_grid<f32>", k_ball_query_grid<float>, grid, dim3(kPgThreads), 0, st, (const float *)centers, m, center_stride,
                   center_offsets, segments, plan, order, cell_offsets, (const float *)packed, r * r, (double)r * (1.0 + kPgSlack), nsample,
                   pad_first, table, counts);
    }
    return D3D_OK;
}

extern "C" int d3d_knn_query_grid(const void *centers, int64_t m, int32_t center_stride, int32_t dtype, const int64_t *center_offsets,
                                  int64_t segments, const D3DPointGridSegment *plan, const int32_t *order, const int64_t *cell_offsets,
                                  const void *packed, int64_t n, int32_t k, int32_t *table, void *dist2, void *stream)
{
    if (k < 1) return D3D_ERR_BAD_ARG;
    if (const int rc = pg_query_check(n, m, segments, center_stride, dtype, center_offsets); rc != D3D_OK) return rc;
    if (k > D3D_KNN_MAX) return D3D_ERR_UNSUPPORTED;
    if (m == 0) return D3D_OK;
    if (!centers || !table || !plan || !cell_offsets || (n > 0 && (!order || !packed))) return D3D_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d3d_divup(m, kPgWaves));
    if (dtype == D3D_F64) {
        D3D_LAUNCH("k_knn_query_grid<f64>", k_knn_query_grid<double>, grid, dim3(kPgThreads), 0, st, (const double *)centers, m, center_stride,
                   center_offsets, segments, plan, order, cell_offsets, (const double *)packed, k, table, (double *)dist2);
    } else {
        D3D_LAUNCH("k_knn_query_grid<f32>", k_knn_query_grid<float>, grid, dim3(kPgThreads), 0, st, (const float *)centers, m, center_stride,
                   center_offsets, segments, plan, order, cell_offsets, (const float *)packed, k, table, (float *)dist2);
    }
    return D3D_OK;
}
