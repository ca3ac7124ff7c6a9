// psample.hip -- the entrance of the point branch on MI355X (gfx950): furthest point sampling and ball query, what PointNet++'s set
// abstraction, PV-RCNN's keypoints, 3DSSD and Voxel R-CNN do first.  Both return indices only, both are defined exactly (the rules
// stand in include/d3d_hip.h), neither uses an atomic.  An extension: the reference has no point sampling.
//
//   d3d_furthest_point_sample  points[n, >= 3], ragged segments -> indices (and the coverage radius squared of every step)
//   d3d_ball_query             points, centres, r -> table[m, nsample] int32 (the first nsample rows inside, ascending; -1: none), counts[m]
//
// k_fps: ONE workgroup of 1024 lanes per segment, one launch for the whole batch; a step of the M dependent ones is
//   every lane: its rows' distance to the last winner, d = min(d, q), and its own best row (strict > in ascending row: the lowest wins);
//   a key that orders like the rule -- the distance's bits (non-negative floats order as integers) above the INVERTED row -- so that
//     a plain maximum is "largest d, lowest row"; 0 = "no row" (a valid key is never 0: ~row > 0 for rows below 2^31 - 1);
//   a wave maximum on DPP steps; the winner's coordinates are read out of the lane and register that hold them (a wave-uniform
//     register, found by scalar branches) and go with the key into the wave's slot of a double-buffered LDS table; ONE barrier (LDS only: it does not
//     wait for the global stores of the outputs);
//   every wave reduces the 16 slots for itself (lanes 0 .. 15 of each DPP row hold one slot each) and reads the winner's coordinates
//     out of the lane that holds them: the next step's centre, in every lane's registers.
// Where a segment's coordinates and d live is its ROUTE, chosen per workgroup from the segment's rows (fps_route, the same function
// d3d_fps_plan answers with):
//   registers  R rows per lane (row = j * 1024 + lane: coalesced), R one of three values per dtype; a segment takes the smallest that holds it;
//   LDS        the largest R, and the rows above R * 1024 in four LDS planes (x, y, z, d; plane[j * 1024 + lane]: conflict-free, and
//              only their owner touches them: no barrier);
//   streaming  any size: coordinates from global memory every step (L2 for what fits), d in the workspace; still one workgroup.
// All routes are inlined into one kernel per dtype: its registers are the largest route's (no scratch: tools/kernel_resources.py),
// its LDS the LDS route's.  A workgroup of 1024 lanes owns a CU whatever it declares, so the small routes lose nothing by it.
//
// k_ball_query: one wavefront per centre walks its segment 4 x 64 rows at a time (four tiles loaded before the first is judged);
// q < r2, a ballot, the count of the lower lanes' bits is the slot: every slot is written once, in order, without a sort.  The walk
// ends (wave-uniform) once nsample rows are found; the same wave writes the padding.  O(m n) per segment by design: see DESIGN.md.
//
// And the way back up, what a feature-propagation layer starts with:
//   d3d_knn_query              points, centres, k -> table[m, k] int32 (ascending (q, row); -1: none), dist2[m, k]
//   d3d_knn_weights            table, dist2 -> the normalised inverse-distance weights[m, k] (three_nn's 1 / (dist + eps))
// k_knn_query: the same walk, a wavefront per centre; the k best so far are kept sorted across the lanes (see the kernel).  The fold
// that uses table and weights is vinterp.hip's (d3d_knn_interp_forward / _backward).
#include "common.hpp"
#include "pquery.hpp"

#include <cmath>
#include <limits>

namespace {

constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / kWave;
constexpr int kFpsLdsBytes = 128 * 1024;       // the four planes of the LDS route (+ the slots: 160 KiB per workgroup on gfx950)
constexpr int64_t kPsRowMax = 0x7fffffffll;
constexpr int kBqThreads = 256;
constexpr int kBqWaves = kBqThreads / kWave;
constexpr int kBqAhead = 4;                    // tiles of 64 rows in flight per wavefront
constexpr int kBqMaxSample = 1024;

// rows per lane of the three register routes; rows per lane the LDS planes add: kFpsLdsBytes / (4 planes * 1024 lanes * sizeof(T))
template <typename T> struct FpsShape;
template <> struct FpsShape<float> {
    static constexpr int kR0 = 1, kR1 = 4, kR2 = 16, kLds = kFpsLdsBytes / (4 * kFpsThreads * 4);
};
template <> struct FpsShape<double> {
    static constexpr int kR0 = 1, kR1 = 2, kR2 = 8, kLds = kFpsLdsBytes / (4 * kFpsThreads * 8);
};

// segment rows -> route; *capacity = the rows that route holds
template <typename T> __host__ __device__ inline int fps_route(int64_t n, int64_t *capacity)
{
    typedef FpsShape<T> S;
    const int64_t cap[5] = {(int64_t)S::kR0 * kFpsThreads, (int64_t)S::kR1 * kFpsThreads, (int64_t)S::kR2 * kFpsThreads,
                            (int64_t)(S::kR2 + S::kLds) * kFpsThreads, kPsRowMax};
    int r = 0;
    while (r < D3D_FPS_ROUTE_STREAM && n > cap[r]) r++;
    if (capacity) *capacity = cap[r];
    return r;
}

__device__ __forceinline__ void ps_lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ---------------------------------------------------------------- the key
// fp32: one 64-bit word {distance bits : 32 | ~row : 32}; fp64: the 64 distance bits and ~row beside them
struct FpsKey64 {
    uint64_t d;
    uint32_t inv;
};
template <typename T> struct FpsKeyOf;
template <> struct FpsKeyOf<float> { typedef uint64_t type; };
template <> struct FpsKeyOf<double> { typedef FpsKey64 type; };

__device__ __forceinline__ uint64_t key_make(float d, uint32_t row) { return ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)~row; }
__device__ __forceinline__ FpsKey64 key_make(double d, uint32_t row) { return FpsKey64{(uint64_t)__double_as_longlong(d), (uint32_t)~row}; }
__device__ __forceinline__ void key_zero(uint64_t &k) { k = 0; }
__device__ __forceinline__ void key_zero(FpsKey64 &k) { k.d = 0, k.inv = 0; }
__device__ __forceinline__ bool key_gt(uint64_t a, uint64_t b) { return a > b; }
__device__ __forceinline__ bool key_gt(const FpsKey64 &a, const FpsKey64 &b) { return a.d > b.d || (a.d == b.d && a.inv > b.inv); }
__device__ __forceinline__ bool key_eq(uint64_t a, uint64_t b) { return a == b; }
__device__ __forceinline__ bool key_eq(const FpsKey64 &a, const FpsKey64 &b) { return a.d == b.d && a.inv == b.inv; }
__device__ __forceinline__ bool key_none(uint64_t k) { return k == 0; }
__device__ __forceinline__ bool key_none(const FpsKey64 &k) { return k.inv == 0; }
__device__ __forceinline__ uint32_t key_row(uint64_t k) { return ~(uint32_t)k; }
__device__ __forceinline__ uint32_t key_row(const FpsKey64 &k) { return ~k.inv; }
__device__ __forceinline__ float key_dist(uint64_t k, float) { return __uint_as_float((uint32_t)(k >> 32)); }
__device__ __forceinline__ double key_dist(const FpsKey64 &k, double) { return __longlong_as_double((long long)k.d); }
// (a lane without a source, and every lane of a masked row, reads the zero key: the identity of the maximum)
template <int CTRL, int ROW_MASK> __device__ __forceinline__ uint64_t key_dpp(uint64_t k) { return d3d_dpp_u64<CTRL, ROW_MASK>(k); }
template <int CTRL, int ROW_MASK> __device__ __forceinline__ FpsKey64 key_dpp(const FpsKey64 &k)
{
    return FpsKey64{d3d_dpp_u64<CTRL, ROW_MASK>(k.d), d3d_dpp_u32<CTRL, ROW_MASK>(k.inv)};
}
using ::wave_readlane;                              // (the overload for the key must not hide common.hpp's)
__device__ __forceinline__ FpsKey64 wave_readlane(const FpsKey64 &k, int lane) { return FpsKey64{wave_readlane(k.d, lane), wave_readlane(k.inv, lane)}; }

#define D3D_KEY_STEP(CTRL, MASK)                   \
    {                                              \
        const K o_ = key_dpp<CTRL, MASK>(k);       \
        if (key_gt(o_, k)) k = o_;                 \
    }
// the maximum over each DPP row of 16 lanes, in the row's last lane
template <typename K> __device__ __forceinline__ K key_row_max(K k)
{
    D3D_KEY_STEP(0x111, 0xf) D3D_KEY_STEP(0x112, 0xf) D3D_KEY_STEP(0x114, 0xf) D3D_KEY_STEP(0x118, 0xf)
    return k;
}
// the maximum over the wavefront, in every lane (wave-uniform)
template <typename K> __device__ __forceinline__ K key_wave_max(K k)
{
    k = key_row_max(k);
    D3D_KEY_STEP(0x142, 0xa) D3D_KEY_STEP(0x143, 0xc)
    return wave_readlane(k, kWave - 1);
}
#undef D3D_KEY_STEP

template <typename T> struct FpsSlot {
    typename FpsKeyOf<T>::type key;
    T x, y, z;
};

// A lane's candidate of one step: the best of its rows so far.  d < 0: none yet.  row: the row MINUS the lane's number (a constant of
// the unrolled loops: no register per row).
template <typename T> struct FpsBest {
    T d;
    uint32_t row;
};

// one row against the last winner (cx, cy, cz), then against the lane's best.  d < 0 marks an excluded row: q >= 0 (or NaN) never
// goes below it, and it never beats a best that starts at -1.
template <typename T> __device__ __forceinline__ void fps_row(T x, T y, T z, T &d, uint32_t row, T cx, T cy, T cz, FpsBest<T> &b)
{
    const T dx = x - cx, dy = y - cy, dz = z - cz;
    const T q = ((dx * dx) + (dy * dy)) + (dz * dz);
    if (q < d) d = q;
    if (d > b.d) b.d = d, b.row = row;
}

// The end of a step, after every lane has its best: -> the winner's coordinates in (cx, cy, cz) of every lane; lane 0 of the
// workgroup writes the step's outputs.  All lanes of the workgroup call it (one barrier inside).  fetch(row, x, y, z): the
// coordinates of one of THIS wavefront's rows, `row` wave-uniform -- a lane carries no coordinates of its best along (three selects
// per row and step); the wave's winner is looked up once.
template <typename T, class Fetch>
__device__ __forceinline__ void fps_elect(const FpsBest<T> &b, int64_t s, int64_t row0, FpsSlot<T> (*slots)[kFpsWaves], int64_t *idx_out,
                                          T *dist_out, T &cx, T &cy, T &cz, Fetch &&fetch)
{
    typedef typename FpsKeyOf<T>::type K;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    K k;
    key_zero(k);
    if (!(b.d < (T)0)) k = key_make(b.d, b.row + threadIdx.x);
    const K wmax = key_wave_max(k);
    T wx = (T)0, wy = (T)0, wz = (T)0;
    if (!key_none(wmax)) fetch(key_row(wmax), wx, wy, wz);                      // (wave-uniform branch)
    FpsSlot<T> *const buf = slots[s & 1];
    if (lane == 0) {
        buf[wave].key = wmax;
        buf[wave].x = wx, buf[wave].y = wy, buf[wave].z = wz;
    }
    ps_lds_barrier();
    const FpsSlot<T> mine = buf[lane & (kFpsWaves - 1)];
    const K win = wave_readlane(key_row_max(mine.key), kWave - 1);
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)__ballot(key_eq(mine.key, win))) - 1);
    cx = wave_readlane(mine.x, src), cy = wave_readlane(mine.y, src), cz = wave_readlane(mine.z, src);
    if (threadIdx.x == 0) {
        const bool none = key_none(win);                                       // every row of the segment is excluded
        idx_out[s] = row0 + (none ? 0 : (int64_t)key_row(win));
        if (dist_out) dist_out[s] = none ? std::numeric_limits<T>::quiet_NaN() : key_dist(win, (T)0);
    }
}

// (x, y, z)[j] of lane l, j and l wave-uniform: scalar branches down to the register (an indexed read of the arrays would put
// them into scratch memory)
template <typename T, int LO, int HI>
__device__ __forceinline__ void fps_pick(const T *x, const T *y, const T *z, int j, int l, T &ox, T &oy, T &oz)
{
    if constexpr (HI - LO == 1) {
        ox = wave_readlane(x[LO], l), oy = wave_readlane(y[LO], l), oz = wave_readlane(z[LO], l);
    } else {
        constexpr int MID = (LO + HI) / 2;
        if (j < MID) fps_pick<T, LO, MID>(x, y, z, j, l, ox, oy, oz);
        else fps_pick<T, MID, HI>(x, y, z, j, l, ox, oy, oz);
    }
}

// a row of the segment as a route keeps it: excluded rows and the lanes past the end carry d = -1
template <typename T> __device__ __forceinline__ void fps_load(const T *seg, int32_t stride, int64_t n, int64_t row, T &x, T &y, T &z, T &d)
{
    x = y = z = (T)0, d = (T)-1;
    if (row < n) {
        const T *p = seg + row * stride;
        const T px = p[0], py = p[1], pz = p[2];
        if (ps_finite3(px, py, pz)) x = px, y = py, z = pz, d = std::numeric_limits<T>::infinity();
    }
}

// registers (and LDS planes above R * 1024 rows)
template <typename T, int R, bool LDS>
__device__ __forceinline__ void fps_chip(const T *seg, int32_t stride, int64_t n, int64_t m, int64_t row0, int64_t *idx_out, T *dist_out,
                                         T *planes, FpsSlot<T> (*slots)[kFpsWaves])
{
    constexpr int kPlane = FpsShape<T>::kLds * kFpsThreads;
    const int t = threadIdx.x;
    T x[R], y[R], z[R], d[R];
#pragma unroll
    for (int j = 0; j < R; j++) fps_load(seg, stride, n, (int64_t)j * kFpsThreads + t, x[j], y[j], z[j], d[j]);
    int nl = 0;
    if constexpr (LDS) {
        nl = (int)((n - (int64_t)R * kFpsThreads + kFpsThreads - 1) / kFpsThreads);   // <= FpsShape<T>::kLds by the route's capacity
        for (int j = 0; j < nl; j++) {
            T lx, ly, lz, ld;
            fps_load(seg, stride, n, (int64_t)(R + j) * kFpsThreads + t, lx, ly, lz, ld);
            const int at = j * kFpsThreads + t;
            planes[at] = lx, planes[kPlane + at] = ly, planes[2 * kPlane + at] = lz, planes[3 * kPlane + at] = ld;
        }
    }
    // row j * 1024 + t lives in lane t % 64 of wave t / 64: register j (a wave-uniform index), or row j - R of the planes
    auto fetch = [&](uint32_t row, T &ox, T &oy, T &oz) {
        const int j = __builtin_amdgcn_readfirstlane((int)(row / kFpsThreads)), l = __builtin_amdgcn_readfirstlane((int)(row & (kWave - 1)));
        if (!LDS || j < R) {
            fps_pick<T, 0, R>(x, y, z, j, l, ox, oy, oz);
        } else {
            const int at = (j - R) * kFpsThreads + (int)(row & (kFpsThreads - 1));
            ox = planes[at], oy = planes[kPlane + at], oz = planes[2 * kPlane + at];
        }
    };
    // before step 0 there is no winner: against NaN no q is below any d
    T cx = std::numeric_limits<T>::quiet_NaN(), cy = cx, cz = cx;
    for (int64_t s = 0; s < m; s++) {
        FpsBest<T> b = {(T)-1, 0u};
#pragma unroll
        for (int j = 0; j < R; j++) fps_row(x[j], y[j], z[j], d[j], (uint32_t)(j * kFpsThreads), cx, cy, cz, b);
        if constexpr (LDS) {
#pragma unroll 1
            for (int j = 0; j < nl; j++) {
                const int at = j * kFpsThreads + t;
                T ld = planes[3 * kPlane + at];
                const T was = ld;
                fps_row(planes[at], planes[kPlane + at], planes[2 * kPlane + at], ld, (uint32_t)((R + j) * kFpsThreads), cx, cy, cz, b);
                if (ld < was) planes[3 * kPlane + at] = ld;
            }
        }
        fps_elect(b, s, row0, slots, idx_out, dist_out, cx, cy, cz, fetch);
    }
}

// any size: coordinates from global memory, d in dws[n] (each element is its owner lane's alone)
template <typename T>
__device__ __forceinline__ void fps_stream(const T *seg, int32_t stride, int64_t n, int64_t m, int64_t row0, int64_t *idx_out, T *dist_out,
                                           T *dws, FpsSlot<T> (*slots)[kFpsWaves])
{
    const int t = threadIdx.x;
    auto fetch = [&](uint32_t row, T &ox, T &oy, T &oz) {
        const T *p = seg + (int64_t)row * stride;
        ox = p[0], oy = p[1], oz = p[2];
    };
    T cx = std::numeric_limits<T>::quiet_NaN(), cy = cx, cz = cx;
    for (int64_t s = 0; s < m; s++) {
        FpsBest<T> b = {(T)-1, 0u};
#pragma unroll 4
        for (int64_t i = t; i < n; i += kFpsThreads) {
            T px, py, pz, d;
            if (s == 0) {
                fps_load(seg, stride, n, i, px, py, pz, d);
                dws[i] = d;
            } else {
                const T *p = seg + i * stride;
                px = p[0], py = p[1], pz = p[2], d = dws[i];                    // (an excluded row: q is NaN or >= 0, never below -1)
            }
            const T was = d;
            fps_row(px, py, pz, d, (uint32_t)(i - t), cx, cy, cz, b);
            if (d < was) dws[i] = d;
        }
        fps_elect(b, s, row0, slots, idx_out, dist_out, cx, cy, cz, fetch);
    }
}

template <typename T>
__global__ __launch_bounds__(kFpsThreads) void k_fps(const T *__restrict__ points, int32_t stride, const int64_t *__restrict__ point_offsets,
                                                     const int64_t *__restrict__ sample_offsets, int64_t *__restrict__ indices,
                                                     T *__restrict__ distances, T *__restrict__ dws)
{
    typedef FpsShape<T> S;
    __shared__ __attribute__((aligned(16))) T planes[kFpsLdsBytes / sizeof(T)];
    __shared__ FpsSlot<T> slots[2][kFpsWaves];
    const int64_t p0 = point_offsets[blockIdx.x], n = point_offsets[blockIdx.x + 1] - p0;
    const int64_t s0 = sample_offsets[blockIdx.x], m = sample_offsets[blockIdx.x + 1] - s0;
    if (m <= 0) return;
    int64_t *const idx_out = indices + s0;
    T *const dist_out = distances ? distances + s0 : nullptr;
    if (n <= 0 || n > kPsRowMax) {             // refused by the caller; a segment without rows has nothing to name
        for (int64_t s = threadIdx.x; s < m; s += kFpsThreads) {
            idx_out[s] = -1;
            if (dist_out) dist_out[s] = std::numeric_limits<T>::quiet_NaN();
        }
        return;
    }
    const T *const seg = points + p0 * stride;
    switch (fps_route<T>(n, nullptr)) {
    case 0: fps_chip<T, S::kR0, false>(seg, stride, n, m, p0, idx_out, dist_out, planes, slots); break;
    case 1: fps_chip<T, S::kR1, false>(seg, stride, n, m, p0, idx_out, dist_out, planes, slots); break;
    case 2: fps_chip<T, S::kR2, false>(seg, stride, n, m, p0, idx_out, dist_out, planes, slots); break;
    case D3D_FPS_ROUTE_LDS: fps_chip<T, S::kR2, true>(seg, stride, n, m, p0, idx_out, dist_out, planes, slots); break;
    default: fps_stream<T>(seg, stride, n, m, p0, idx_out, dist_out, dws + p0, slots); break;
    }
}

// ---------------------------------------------------------------- ball query
template <typename T>
__global__ __launch_bounds__(kBqThreads) void k_ball_query(const T *__restrict__ points, int64_t n, int32_t pstride, const T *__restrict__ centers,
                                                           int64_t m, int32_t cstride, const int64_t *__restrict__ point_offsets,
                                                           const int64_t *__restrict__ center_offsets, int64_t segments, T r2, int32_t nsample,
                                                           int32_t pad_first, int32_t *__restrict__ table, int32_t *__restrict__ counts)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t c = (int64_t)blockIdx.x * kBqWaves + threadIdx.x / kWave;
    if (c >= m) return;
    int64_t p0 = 0, p1 = n;
    if (center_offsets) {                      // the segment b of the centre: center_offsets[b] <= c < center_offsets[b + 1]
        const int64_t lo = ps_segment_of(center_offsets, segments, c);
        p0 = point_offsets[lo], p1 = point_offsets[lo + 1];
    }
    const T *const q0 = centers + c * cstride;
    const T cx = q0[0], cy = q0[1], cz = q0[2];
    int32_t *const row = table + c * nsample;
    int found = 0;
    int32_t first = -1;
    for (int64_t base = p0; base < p1 && found < nsample; base += kBqAhead * kWave) {
        bool in[kBqAhead];
#pragma unroll
        for (int u = 0; u < kBqAhead; u++) {
            const int64_t i = base + u * kWave + lane;
            in[u] = false;
            if (i < p1) {
                const T *p = points + i * pstride;
                in[u] = ps_q<T>(p[0], p[1], p[2], cx, cy, cz) < r2;              // false for NaN
            }
        }
#pragma unroll
        for (int u = 0; u < kBqAhead; u++) {
            const unsigned long long vote = __ballot(in[u]);
            if (vote == 0) continue;
            if (first < 0) first = (int32_t)(base + u * kWave + __ffsll((long long)vote) - 1);
            const int slot = found + __popcll(vote & ((1ull << lane) - 1ull));
            if (in[u] && slot < nsample) row[slot] = (int32_t)(base + u * kWave + lane);
            found += __popcll(vote);           // (at most nsample - 1 + 64 * kBqAhead: the walk ends once nsample are found)
        }
    }
    const int count = found < nsample ? found : nsample;
    const int32_t pad = pad_first ? first : -1;                                 // (an empty ball: first is -1)
    for (int slot = count + lane; slot < nsample; slot += kWave) row[slot] = pad;
    if (lane == 0) counts[c] = count;
}

// ---------------------------------------------------------------- k nearest rows
// (the order-keeping key of a candidate and its insertion: pquery.hpp, shared with the grid route of pgrid.hip)
// One wavefront per centre.  The wave holds its best rows so far SORTED ACROSS LANES: lane l the l-th smallest key (all ones while
// fewer than l + 1 candidates were seen); tau = lane k - 1's key, wave-uniform, is what a row has to beat.  The segment is walked
// 4 x 64 rows at a time, as k_ball_query walks it; per tile key < tau and a ballot -- zero for most tiles of an unordered cloud once
// the first few are in, then the tile costs the compare alone.  Every set bit, in ascending lane, is inserted wave-uniformly: the
// key is broadcast, its position is the number of held keys below it, the lanes above take their lower neighbour's key (one wave
// shift), the lane at the position takes the new key, tau is read again and the ballot is taken again over the lanes above.  No LDS,
// no atomics, no workspace; the lanes k .. 63 hold the next best keys, which costs nothing and is never read.
template <typename T>
__global__ __launch_bounds__(kBqThreads) void k_knn_query(const T *__restrict__ points, int64_t n, int32_t pstride, const T *__restrict__ centers,
                                                          int64_t m, int32_t cstride, const int64_t *__restrict__ point_offsets,
                                                          const int64_t *__restrict__ center_offsets, int64_t segments, int32_t k,
                                                          int32_t *__restrict__ table, T *__restrict__ dist2)
{
    typedef typename KnnKeyOf<T>::type K;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t c = (int64_t)blockIdx.x * kBqWaves + threadIdx.x / kWave;
    if (c >= m) return;
    int64_t p0 = 0, p1 = n;
    if (center_offsets) {                      // the segment b of the centre: center_offsets[b] <= c < center_offsets[b + 1]
        const int64_t lo = ps_segment_of(center_offsets, segments, c);
        p0 = point_offsets[lo], p1 = point_offsets[lo + 1];
    }
    const T *const q0 = centers + c * cstride;
    const T cx = q0[0], cy = q0[1], cz = q0[2];
    K held, tau;
    knn_clear(held), knn_clear(tau);
    for (int64_t base = p0; base < p1; base += kBqAhead * kWave) {
        K key[kBqAhead];
#pragma unroll
        for (int u = 0; u < kBqAhead; u++) {
            const int64_t i = base + u * kWave + lane;
            knn_clear(key[u]);
            if (i < p1) {
                const T *p = points + i * pstride;
                const T q = ps_q<T>(p[0], p[1], p[2], cx, cy, cz);
                if (q == q) key[u] = knn_make(q, (uint32_t)i);                  // (a NaN q: no candidate)
            }
        }
#pragma unroll
        for (int u = 0; u < kBqAhead; u++) knn_insert_tile(key[u], held, tau, lane, k);
    }
    if (lane < k) {
        const bool none = knn_none(held);
        table[c * k + lane] = none ? -1 : (int32_t)knn_row(held);
        if (dist2) dist2[c * k + lane] = none ? std::numeric_limits<T>::infinity() : knn_dist(held, (T)0);
    }
}

// one lane per table row: the inverse-distance weights of its present entries, normalised by their sum in ascending column
template <typename T>
__global__ __launch_bounds__(kBqThreads) void k_knn_weights(const int32_t *__restrict__ table, const T *__restrict__ dist2, int64_t m, int32_t k,
                                                            int32_t power, T eps, T *__restrict__ weights)
{
    const int64_t r = (int64_t)blockIdx.x * kBqThreads + threadIdx.x;
    if (r >= m) return;
    const int32_t *const t = table + r * k;
    const T *const q = dist2 + r * k;
    T *const w = weights + r * k;
    auto u_of = [&](int j) { return (T)1 / ((power == 1 ? sqrt(q[j]) : q[j]) + eps); };
    T s = (T)0;
    for (int j = 0; j < k; j++)
        if (t[j] >= 0) s = s + u_of(j);
    const bool ok = s > (T)0 && s < std::numeric_limits<T>::infinity();          // false for NaN
    for (int j = 0; j < k; j++) w[j] = (ok && t[j] >= 0) ? u_of(j) / s : (T)0;
}

bool ps_dtype_ok(int32_t dtype) { return dtype == D3D_F32 || dtype == D3D_F64; }

// the one layout of the FPS workspace: d of every row, for the segments on the streaming route
struct FpsWs {
    void *d;
};
FpsWs fps_carve(WsCarver &w, int64_t n, int32_t dtype)
{
    FpsWs r;
    r.d = w.take<char>((size_t)(n > 1 ? n : 1) * (dtype == D3D_F64 ? 8 : 4));
    return r;
}

}  // namespace

extern "C" size_t d3d_fps_workspace_bytes(int64_t n, int64_t segments, int32_t dtype)
{
    (void)segments;
    WsCarver w(nullptr, 0);
    fps_carve(w, n > 0 ? n : 0, dtype);
    return w.off;
}

extern "C" int d3d_fps_plan(int64_t segment_rows, int32_t dtype, int32_t *route, int32_t *capacity)
{
    if (segment_rows < 0 || !route || !capacity) return D3D_ERR_BAD_ARG;
    if (!ps_dtype_ok(dtype) || segment_rows > kPsRowMax) return D3D_ERR_UNSUPPORTED;
    int64_t cap = 0;
    *route = dtype == D3D_F64 ? fps_route<double>(segment_rows, &cap) : fps_route<float>(segment_rows, &cap);
    *capacity = (int32_t)cap;
    return D3D_OK;
}

extern "C" int d3d_furthest_point_sample(const void *points, int64_t n, int32_t row_stride, int32_t dtype, const int64_t *point_offsets,
                                         const int64_t *sample_offsets, int64_t segments, int64_t *indices, void *distances, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    if (n < 0 || segments < 0 || row_stride < 3) return D3D_ERR_BAD_ARG;
    if (!ps_dtype_ok(dtype) || segments > kPsRowMax) return D3D_ERR_UNSUPPORTED;
    if (segments == 0) return D3D_OK;
    if (!point_offsets || !sample_offsets || !indices || (n > 0 && !points)) return D3D_ERR_BAD_ARG;
    WsCarver w(workspace, workspace_bytes);
    const FpsWs ws = fps_carve(w, n, dtype);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == D3D_F64) {
        D3D_LAUNCH("k_fps<f64>", k_fps<double>, dim3((unsigned)segments), dim3(kFpsThreads), 0, st, (const double *)points, row_stride,
                   point_offsets, sample_offsets, indices, (double *)distances, (double *)ws.d);
    } else {
        D3D_LAUNCH("k_fps<f32>", k_fps<float>, dim3((unsigned)segments), dim3(kFpsThreads), 0, st, (const float *)points, row_stride,
                   point_offsets, sample_offsets, indices, (float *)distances, (float *)ws.d);
    }
    return D3D_OK;
}

extern "C" int d3d_ball_query(const void *points, int64_t n, int32_t point_stride, const void *centers, int64_t m, int32_t center_stride,
                              int32_t dtype, const int64_t *point_offsets, const int64_t *center_offsets, int64_t segments, double radius,
                              int32_t nsample, int32_t pad_first, int32_t *table, int32_t *counts, void *stream)
{
    if (n < 0 || m < 0 || segments < 0 || point_stride < 3 || center_stride < 3 || nsample < 1 || nsample > kBqMaxSample) return D3D_ERR_BAD_ARG;
    if (!(radius > 0) || !std::isfinite(radius) || (point_offsets == nullptr) != (center_offsets == nullptr)) return D3D_ERR_BAD_ARG;
    if (point_offsets && segments < 1 && m > 0) return D3D_ERR_BAD_ARG;
    if (!ps_dtype_ok(dtype) || n > kPsRowMax || m > kPsRowMax) return D3D_ERR_UNSUPPORTED;
    if (m == 0) return D3D_OK;
    if (!centers || !table || !counts || (n > 0 && !points)) return D3D_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d3d_divup(m, kBqWaves));
    if (dtype == D3D_F64) {
        const double r = radius;
        D3D_LAUNCH("k_ball_query<f64>", k_ball_query<double>, grid, dim3(kBqThreads), 0, st, (const double *)points, n, point_stride,
                   (const double *)centers, m, center_stride, point_offsets, center_offsets, segments, r * r, nsample, pad_first, table, counts);
    } else {
        const float r = (float)radius;
        D3D_LAUNCH("k_ball_query<f32>", k_ball_query<float>, grid, dim3(kBqThreads), 0, st, (const float *)points, n, point_stride,
                   (const float *)centers, m, center_stride, point_offsets, center_offsets, segments, r * r, nsample, pad_first, table, counts);
    }
    return D3D_OK;
}

extern "C" int d3d_knn_query(const void *points, int64_t n, int32_t point_stride, const void *centers, int64_t m, int32_t center_stride,
                             int32_t dtype, const int64_t *point_offsets, const int64_t *center_offsets, int64_t segments, int32_t k,
                             int32_t *table, void *dist2, void *stream)
{
    if (n < 0 || m < 0 || segments < 0 || point_stride < 3 || center_stride < 3 || k < 1) return D3D_ERR_BAD_ARG;
    if ((point_offsets == nullptr) != (center_offsets == nullptr)) return D3D_ERR_BAD_ARG;
    if (point_offsets && segments < 1 && m > 0) return D3D_ERR_BAD_ARG;
    if (!ps_dtype_ok(dtype) || n > kPsRowMax || m > kPsRowMax || segments > kPsRowMax || k > D3D_KNN_MAX) return D3D_ERR_UNSUPPORTED;
    if (m == 0) return D3D_OK;
    if (!centers || !table || (n > 0 && !points)) return D3D_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d3d_divup(m, kBqWaves));
    if (dtype == D3D_F64) {
        D3D_LAUNCH("k_knn_query<f64>", k_knn_query<double>, grid, dim3(kBqThreads), 0, st, (const double *)points, n, point_stride,
                   (const double *)centers, m, center_stride, point_offsets, center_offsets, segments, k, table, (double *)dist2);
    } else {
        D3D_LAUNCH("k_knn_query<f32>", k_knn_query<float>, grid, dim3(kBqThreads), 0, st, (const float *)points, n, point_stride,
                   (const float *)centers, m, center_stride, point_offsets, center_offsets, segments, k, table, (float *)dist2);
    }
    return D3D_OK;
}

extern "C" int d3d_knn_weights(const int32_t *table, const void *dist2, int64_t m, int32_t k, int32_t dtype, int32_t power, double eps,
                               void *weights, void *stream)
{
    if (m < 0 || k < 1 || (power != 1 && power != 2)) return D3D_ERR_BAD_ARG;
    if (!ps_dtype_ok(dtype) || k > D3D_KNN_MAX || m > kPsRowMax / k) return D3D_ERR_UNSUPPORTED;
    const double e = dtype == D3D_F64 ? eps : (double)(float)eps;               // eps as the kernel adds it
    if (!(e >= 0) || !std::isfinite(e)) return D3D_ERR_BAD_ARG;
    if (m == 0) return D3D_OK;
    if (!table || !dist2 || !weights) return D3D_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)d3d_divup(m, kBqThreads));
    if (dtype == D3D_F64) {
        D3D_LAUNCH("k_knn_weights<f64>", k_knn_weights<double>, grid, dim3(kBqThreads), 0, st, table, (const double *)dist2, m, k, power, e,
                   (double *)weights);
    } else {
        D3D_LAUNCH("k_knn_weights<f32>", k_knn_weights<float>, grid, dim3(kBqThreads), 0, st, table, (const float *)dist2, m, k, power, (float)e,
                   (float *)weights);
    }
    return D3D_OK;
}
