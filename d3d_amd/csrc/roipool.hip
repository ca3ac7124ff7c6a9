// roipool.hip -- the points of every RoI binned into the cells of its own rotated grid on MI355X (gfx950): the table behind Part-A2's
// roiaware_pool3d (pts_idx_of_voxels) and, with one cell and the cyclic fill, behind PointRCNN's roipoint_pool3d.  An extension: the
// reference has crop_points (a bool[M, N] mask) and nothing that bins.
//
//   d3d_roi_grid_table   points[n, >= 3], boxes[m, 7], out_size (ox, oy, oz), P -> table[m, G, P] int32 (-1: none), counts[m, G], inside[m]
//
// Membership is contains3 of geom.hpp, the test of d3d_crop_3dr, on finite points; the cell comes from the box's local coordinates and
// is clamped (the exact rule: include/d3d_hip.h).  A cell's entries are its first P members in ascending row: no float atomics, no
// [m, n] mask, no sort, the same bits on every run and for every launch shape.
//
// k_roi_grid: ONE workgroup of 8 wavefronts per box, one launch.  The box's segment is taken in ROUNDS of 8 slabs of 256 rows
// (d3d_roi_grid_plan), two barriers per round:
//   walk     wavefront w loads slab w of the round -- 4 x 64 rows, k_ball_query's loads -- and judges it.  near3 (z interval, the
//            rectangle's bounding box) and a ballot drop the tiles without a candidate -- almost all of them; candidates get the full
//            test and a cell.  The members go, in row order, into the wavefront's QUEUE in LDS (row, cell; the slot is the count so
//            far plus the lower lanes' bits of the ballot).  A queue holds a whole slab: it cannot overflow.
//   place    where the round has a member at all: every wavefront reads the eight queues in slab order, 64 entries at a time, and
//            keeps the entries of ITS cells (cell % 8 == w).  The lanes of one cell are peeled off together, their slot is the cell's
//            count (LDS, touched by its owner wavefront only) plus their rank among them, the first P are stored.  Rounds, slabs and
//            queue entries are all taken in ascending row, so every cell fills in ascending row: nothing to stitch, nothing to sort.
//   pad      after the last round, all wavefronts: counts, and the slots past a cell's count (-1, or the cell's entries again,
//            cyclically) -- every slot of the table is written by this launch exactly once (the cyclic fill reads back what `place`
//            stored: same workgroup, after a barrier).  No memset of the m * G * P words.
#include "common.hpp"
#include "geom.hpp"

namespace {

constexpr int kRgThreads = 512;
constexpr int kRgWaves = kRgThreads / kWave;
constexpr int kRgAhead = 4;                    // tiles of 64 rows in flight per wavefront
constexpr int kRgSlab = kRgAhead * kWave;      // rows a wavefront judges per round; its queue holds as many members
constexpr int kRgRound = kRgWaves * kRgSlab;   // rows the workgroup takes between two barriers
constexpr int kRgMaxCells = 4096;              // 16^3: the counters are 16 KiB of LDS
constexpr int kRgMaxPoints = 1024;
constexpr int64_t kRgRowMax = 0x7fffffffll;

// what a cell is computed from: the box row, the sine and cosine make_geom took, the grid
struct RgFrame {
    float bx, by, bz, lx, ly, lz, s, c;
    int ox, oy, oz;
};

__device__ __forceinline__ int rg_axis(float t, int o)
{
    return !(t >= 0.f) ? 0 : (int)fminf(t, (float)(o - 1));                    // (NaN -> 0; saturated before the conversion)
}

__device__ __forceinline__ int rg_cell(const RgFrame &f, float x, float y, float z)
{
    const float dx = x - f.bx, dy = y - f.by, dz = z - f.bz;
    const float u = dx * f.c + dy * f.s, v = dy * f.c - dx * f.s;
    const float tx = (u / f.lx + 0.5f) * (float)f.ox, ty = (v / f.ly + 0.5f) * (float)f.oy, tz = (dz / f.lz + 0.5f) * (float)f.oz;
    return (rg_axis(tx, f.ox) * f.oy + rg_axis(ty, f.oy)) * f.oz + rg_axis(tz, f.oz);
}

__device__ __forceinline__ bool rg_finite3(float x, float y, float z)
{
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;   // false for NaN
}

// One wavefront over the rows [s0, s1): take(member, row, cell) is called by all 64 lanes, tile after tile in ascending row, for
// every tile that holds a candidate of the cheap test (the others hold no member).
template <class Take>
__device__ __forceinline__ void rg_walk(const float *__restrict__ points, int32_t pstride, int64_t s0, int64_t s1, const Box3 &box,
                                        const RgFrame &f, int lane, Take &&take)
{
    for (int64_t base = s0; base < s1; base += kRgAhead * kWave) {
        float x[kRgAhead], y[kRgAhead], z[kRgAhead];
        bool near[kRgAhead];
#pragma unroll
        for (int u = 0; u < kRgAhead; u++) {
            const int64_t i = base + u * kWave + lane;
            near[u] = false;
            x[u] = y[u] = z[u] = 0.f;
            if (i < s1) {
                const float *p = points + i * pstride;
                x[u] = p[0], y[u] = p[1], z[u] = p[2];
                near[u] = near3(box, x[u], y[u], z[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kRgAhead; u++) {
            if (__ballot(near[u]) == 0) continue;                               // (wave-uniform)
            const bool member = near[u] && rg_finite3(x[u], y[u], z[u]) && contains3(box, x[u], y[u], z[u]);
            take(member, (int32_t)(base + u * kWave + lane), member ? rg_cell(f, x[u], y[u], z[u]) : 0);
        }
    }
}

__global__ __launch_bounds__(kRgThreads) void k_roi_grid(const float *__restrict__ points, int64_t n, int32_t pstride,
                                                         const float *__restrict__ boxes, int32_t bstride, int32_t boff,
                                                         const int64_t *__restrict__ point_offsets, const int64_t *__restrict__ box_offsets,
                                                         int64_t segments, int32_t ox, int32_t oy, int32_t oz, int32_t P, int32_t cycle,
                                                         int32_t *table, int32_t *__restrict__ counts, int32_t *__restrict__ inside)
{
    __shared__ uint32_t cnt[kRgMaxCells];                  // members of every cell so far (uncapped); cell c is wavefront c % 8's
    __shared__ int32_t qrow[kRgWaves][kRgSlab];
    __shared__ uint16_t qcell[kRgWaves][kRgSlab];
    __shared__ uint32_t nmem[kRgWaves];                    // members of every slab of the round; at the end: of every wavefront's slabs
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int64_t b = blockIdx.x;
    const int G = ox * oy * oz;
    int64_t p0 = 0, p1 = n;
    if (box_offsets) {                         // the segment s of the box: box_offsets[s] <= b < box_offsets[s + 1]
        int64_t lo = 0, hi = segments;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (box_offsets[mid] <= b) lo = mid;
            else hi = mid;
        }
        p0 = point_offsets[lo], p1 = point_offsets[lo + 1];
    }
    const float *const brow = boxes + b * bstride + boff;
    const Box3 box = load_box3(brow);
    RgFrame f;
    f.bx = brow[0], f.by = brow[1], f.bz = brow[2], f.lx = brow[3], f.ly = brow[4], f.lz = brow[5];
    d3d_sincos(brow[6], &f.s, &f.c);
    f.ox = ox, f.oy = oy, f.oz = oz;
    for (int c = threadIdx.x; c < G; c += kRgThreads) cnt[c] = 0;

    const unsigned long long below = (1ull << lane) - 1ull;
    int32_t *const trow = table + b * (int64_t)G * P;
    volatile uint32_t *const vcnt = cnt;                   // (written by one lane, read by all lanes of the wavefront in the next step)
    auto place = [&](bool member, int32_t row, int cell) {
        unsigned long long todo = __ballot(member);
        while (todo) {                                                          // (wave-uniform) one cell per step
            const int c0 = __builtin_amdgcn_readlane(cell, __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1));
            const bool mine = member && cell == c0;
            const unsigned long long same = __ballot(mine);
            const uint32_t have = vcnt[c0];
            const uint32_t slot = have + (uint32_t)__popcll(same & below);
            if (mine && slot < (uint32_t)P) trow[c0 * P + (int)slot] = row;
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) vcnt[c0] = have + (uint32_t)__popcll(same);
            __builtin_amdgcn_wave_barrier();
            todo &= ~same;
        }
    };
    uint32_t walked = 0;                                   // the members of this wavefront's slabs
    __syncthreads();                                       // (the counters are zero)
    for (int64_t r0 = p0; r0 < p1; r0 += kRgRound) {
        // ---- walk: the members of this wavefront's slab of the round, in row order, into its queue
        const int64_t s0 = r0 + w * kRgSlab < p1 ? r0 + w * kRgSlab : p1, s1 = s0 + kRgSlab < p1 ? s0 + kRgSlab : p1;
        uint32_t nq = 0;
        rg_walk(points, pstride, s0, s1, box, f, lane, [&](bool member, int32_t row, int cell) {
            const unsigned long long vote = __ballot(member);
            const uint32_t pos = nq + (uint32_t)__popcll(vote & below);         // (below kRgSlab: a slab has no more rows)
            if (member) qrow[w][pos] = row, qcell[w][pos] = (uint16_t)cell;
            nq += (uint32_t)__popcll(vote);
        });
        if (lane == 0) nmem[w] = nq;
        walked += nq;
        if (!__syncthreads_or(nq != 0)) continue;          // (block-uniform) a round without a member: the next one
        // ---- place: the queues in slab order, every wavefront its own cells
        for (int ww = 0; ww < kRgWaves; ww++) {
            const uint32_t held = nmem[ww];
            for (uint32_t k0 = 0; k0 < held; k0 += kWave) {
                const bool there = k0 + lane < held;
                const int cell = there ? (int)qcell[ww][k0 + lane] : 0;
                const bool member = there && cell % kRgWaves == w;
                place(member, member ? qrow[ww][k0 + lane] : 0, cell);
            }
        }
        __syncthreads();                                   // (the queues are free again)
    }
    if (lane == 0) nmem[w] = walked;
    __syncthreads();

    // ---- pad: counts, inside, and every slot past a cell's count
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (int ww = 0; ww < kRgWaves; ww++) all += nmem[ww];
        inside[b] = (int32_t)all;
    }
    for (int c = threadIdx.x; c < G; c += kRgThreads) counts[b * G + c] = (int32_t)(cnt[c] < (uint32_t)P ? cnt[c] : (uint32_t)P);
    for (int c = w; c < G; c += kRgWaves) {
        const int k = (int)(cnt[c] < (uint32_t)P ? cnt[c] : (uint32_t)P);
        int32_t *const cell = trow + c * P;
        for (int j = k + lane; j < P; j += kWave) cell[j] = (cycle && k > 0) ? cell[j % k] : -1;
    }
}

}  // namespace

extern "C" int32_t d3d_roi_grid_max_cells(void) { return kRgMaxCells; }

extern "C" int d3d_roi_grid_plan(int64_t segment_rows, int32_t cells, int32_t *tile_rows, int32_t *slab_rows, int32_t *round_rows)
{
    if (segment_rows < 0 || cells < 1 || !tile_rows || !slab_rows || !round_rows) return D3D_ERR_BAD_ARG;
    if (segment_rows > kRgRowMax || cells > kRgMaxCells) return D3D_ERR_UNSUPPORTED;
    *tile_rows = kWave;
    *slab_rows = kRgSlab;
    *round_rows = kRgRound;
    return D3D_OK;
}

extern "C" int d3d_roi_grid_table(const void *points, int64_t n, int32_t point_stride, const void *boxes, int64_t m, int32_t box_stride,
                                  int32_t box_offset, int32_t dtype, const int64_t *point_offsets, const int64_t *box_offsets,
                                  int64_t segments, const int32_t *out_size, int32_t max_points, int32_t pad, int32_t *table,
                                  int32_t *counts, int32_t *inside, void *stream)
{
    if (n < 0 || m < 0 || segments < 0 || point_stride < 3 || box_offset < 0 || box_stride < box_offset + 7) return D3D_ERR_BAD_ARG;
    if ((point_offsets == nullptr) != (box_offsets == nullptr) || (pad != 0 && pad != 1)) return D3D_ERR_BAD_ARG;
    if (point_offsets && segments < 1 && m > 0) return D3D_ERR_BAD_ARG;
    if (!out_size || out_size[0] < 1 || out_size[1] < 1 || out_size[2] < 1) return D3D_ERR_BAD_ARG;
    if (max_points < 1 || max_points > kRgMaxPoints) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 || n > kRgRowMax || m > kRgRowMax || segments > kRgRowMax) return D3D_ERR_UNSUPPORTED;
    if (out_size[0] > kRgMaxCells || out_size[1] > kRgMaxCells || out_size[2] > kRgMaxCells) return D3D_ERR_UNSUPPORTED;
    const int64_t g = (int64_t)out_size[0] * out_size[1] * out_size[2];
    if (g > kRgMaxCells || m > kRgRowMax / (g * max_points)) return D3D_ERR_UNSUPPORTED;
    if (m == 0) return D3D_OK;
    if (!boxes || !table || !counts || !inside || (n > 0 && !points)) return D3D_ERR_BAD_ARG;
    D3D_LAUNCH("k_roi_grid", k_roi_grid, dim3((unsigned)m), dim3(kRgThreads), 0, (hipStream_t)stream, (const float *)points, n, point_stride,
               (const float *)boxes, box_stride, box_offset, point_offsets, box_offsets, segments, out_size[0], out_size[1], out_size[2],
               max_points, pad, table, counts, inside);
    return D3D_OK;
}
