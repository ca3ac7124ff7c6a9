// vdense.hip -- the exit of a sparse backbone on MI355X (gfx950): sparse voxel rows [V, C] into a dense channels-first grid
// [N, C, A, B, D] (spconv's .dense(); viewed [N, C * A, B, D] it is the BEV map of SECOND / CenterPoint / PV-RCNN's RPN) and back, the
// values of a dense tensor at the active sites as [V, C].  Each is the other's gradient.  An extension: the reference stops at the
// voxelizer.
//
//   d3d_vdense_map      coords, batch -> cell[V] (the flat cell of every row) and index[N * P] (the row at every cell, -1: none)
//   d3d_vdense_scatter  feat[V, C], index -> out[N, C, P]       every element written once: a present cell's row, `fill` elsewhere
//   d3d_vdense_gather   dense[N, C, P], index -> out[V, C]      every row written once
//
// Rows are channel-minor, the grid is channel-major: both kernels are a transposition through LDS.  k_vdense: a workgroup owns a
// stretch of kVdTile consecutive cells of ONE sample and loads their index entries (coalesced).  A stretch without a present cell never
// touches the tile: the scatter streams `fill` into the stretch of all C planes, the gather returns.  A SPARSE stretch (at most
// kVdSparse present cells) does not either: the scatter patches the few present elements into the packs of fill it streams, the
// gather reads them where they lie -- staging would load (gather) or fill in LDS (scatter) kVdTile cells per channel for their sake.
// Otherwise, per chunk of kVdChunkBytes / s channels (s = the element size):
//   the ROW side    a lane group per cell, a lane per 16 bytes of the row's chunk (per element where C or the base do not allow), the
//                   way the row kernels of vrow.hpp move rows; eight rows in flight per lane;
//   the PLANE side  a lane per 16 bytes of a channel plane's stretch (per element where P or the base do not allow): 1 KiB per
//                   wave-instruction, whole planes' stretches one after the other.
// The scatter runs row side -> tile -> plane side, the gather plane side -> tile -> row side; elements move as integers of their
// size, so NaN payloads, infinities and -0.0 arrive bit for bit.  No atomics, no workspace, no launch waits on another workgroup.
//
// The tile is channel-major, [chunk][kVdTile] elements, so the plane side moves 16-byte slots (ds_read_b128 / ds_write_b128: any
// permutation of the slots of a 256-byte bank row is conflict-free) and the row side single elements at a stride of kVdTile.  That
// stride is a multiple of the 32 banks: unswizzled, the 8 lanes of a row would meet on one bank.  Instead of padding (a pad that keeps
// columns 16-byte aligned is a multiple of 4 banks and leaves the 8 lanes 4-way) the cell index of channel ch is XORed with
// vd_swizzle(ch) = (((ch / W) ^ ch) & 7) * W, W = 16 / s cells per slot: a multiple of W (slots stay whole) that takes 8 different
// values over the 8 lanes of a row for every element q of their packs.  A 32-lane group of a ds_write_b32 / ds_read_b32 is 4
// consecutive cells x 8 lanes: banks (cell ^ swizzle) mod 32, 32 different ones; fp64 (16-lane groups, two banks per element) and the
// half types (two cells share a dword, 2-way at most: free on a 4-cycle write) come out the same.  The per-element row path (C not
// a multiple of W) puts 32 lanes on one row and is 4-way: the slow path, by contract.
//
// Bytes moved (model): N C P s of grid + V C s of rows + 4 N P of index.
#include "vrow.hpp"

namespace {

constexpr int kVdThreads = 256;
constexpr int kVdTile = 256;                   // cells of a stretch (d3d_vdense_tile_cells)
constexpr int kVdChunkBytes = 128;             // bytes of a row that one pass of the tile takes: 64 / 32 / 16 channels
constexpr int kVdAhead = 8;                    // rows in flight per lane on the row side
constexpr int kVdSparse = 16;                  // a stretch with at most this many present cells moves them element by element
constexpr int64_t kVdMaxStretches = 0x7fffffffll;

template <int S> struct VdWord;
template <> struct VdWord<2> { typedef uint16_t type; };
template <> struct VdWord<4> { typedef uint32_t type; };
template <> struct VdWord<8> { typedef uint64_t type; };

// The barrier of these kernels orders LDS traffic ONLY: workgroups never talk through global memory (rows and grid are each read-only
// or write-only in a launch).  __syncthreads() also waits until every global store of the wavefront is acknowledged, a barrier or two
// per stretch: a few percent of a launch that is mostly fill.
__device__ __forceinline__ void vd_lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int W> __device__ __forceinline__ int vd_swizzle(int ch) { return (((ch / W) ^ ch) & 7) * W; }

// One stretch through the tile (gather: also a sparse stretch, without it).  U: the element as an integer; VR / VP: elements per lane
// and move on the row / plane side (16 / sizeof(U) or 1).  rows = feat (scatter) or out (gather): [V, c]; planes = the stretch's
// first cell in channel 0 of its sample in out (scatter) or dense (gather); sidx = its index entries in LDS (-1 past the end of the
// sample), `present` of them >= 0; live = the stretch's cells.
template <typename U, int VR, int VP, bool GATHER>
__device__ __forceinline__ void vd_stretch(U *__restrict__ rows, const int32_t *sidx, int present, int32_t c, int64_t p, int live, U fill,
                                           U *__restrict__ planes)
{
    constexpr int W = 16 / (int)sizeof(U), CH = kVdChunkBytes / (int)sizeof(U);
    constexpr int G = CH / VR, RPP = kVdThreads / G;           // lanes of a row; rows of the tile per pass of the workgroup
    constexpr int SPC = kVdTile / VP;                          // packs of a plane's stretch
    typedef RowPack<U, VR> PR;
    typedef RowPack<U, VP> PP;
    __shared__ __attribute__((aligned(16))) U tile[CH * kVdTile];
    __shared__ int32_t slist[kVdSparse];                       // (gather) the present cells of a sparse stretch, in any order
    __shared__ int scount;
    const int t = threadIdx.x;

    // gather, a SPARSE stretch: a lane per (present cell, channel) reads its element where it lies and writes rows coalesced
    if (GATHER && present <= kVdSparse) {
        if (t == 0) scount = 0;
        vd_lds_barrier();
        if (sidx[t] >= 0) slist[atomicAdd(&scount, 1)] = t;
        vd_lds_barrier();
        for (int i = t; i < present * c; i += kVdThreads) {
            const int cell = slist[i / c], ch = i % c;
            rows[(int64_t)sidx[cell] * c + ch] = planes[(int64_t)ch * p + cell];
        }
        return;
    }

    const int g = t % G, rslot = t / G;
    for (int c0 = 0; c0 < c; c0 += CH) {
        const int chn = c - c0 < CH ? c - c0 : CH;                                         // channels of this chunk
        const int cr = g * VR;                                                             // this lane's channels of the chunk
        // plane side <-> tile
        auto plane_side = [&]() {
            for (int i = t; i < chn * SPC; i += kVdThreads) {
                const int ch = i / SPC, cell = (i % SPC) * VP;
                if (cell >= live) continue;
                U *const at = tile + ch * kVdTile + (cell ^ vd_swizzle<W>(ch));
                U *const far = planes + (int64_t)(c0 + ch) * p + cell;
                if constexpr (GATHER) *(PP *)at = *(const PP *)far;
                else *(PP *)far = *(const PP *)at;
            }
        };
        // row side <-> tile: row = pass * RPP + rslot
        auto row_side = [&]() {
            if (cr >= chn) return;
#pragma unroll 1
            for (int pass = 0; pass < G; pass += kVdAhead) {
                PR x[kVdAhead];
                int32_t id[kVdAhead];
#pragma unroll
                for (int a = 0; a < kVdAhead; a++) id[a] = sidx[(pass + a) * RPP + rslot];
                if constexpr (!GATHER) {
#pragma unroll
                    for (int a = 0; a < kVdAhead; a++) {
#pragma unroll
                        for (int q = 0; q < VR; q++) x[a].v[q] = fill;
                        if (id[a] >= 0) x[a] = *(const PR *)(rows + (int64_t)id[a] * c + c0 + cr);
                    }
                }
#pragma unroll
                for (int a = 0; a < kVdAhead; a++) {
                    const int cell = (pass + a) * RPP + rslot;
#pragma unroll
                    for (int q = 0; q < VR; q++) {
                        U *const at = tile + (cr + q) * kVdTile + (cell ^ vd_swizzle<W>(cr + q));
                        if constexpr (GATHER) x[a].v[q] = *at;
                        else *at = x[a].v[q];
                    }
                }
                if constexpr (GATHER) {
#pragma unroll
                    for (int a = 0; a < kVdAhead; a++)
                        if (id[a] >= 0) *(PR *)(rows + (int64_t)id[a] * c + c0 + cr) = x[a];
                }
            }
        };
        if constexpr (GATHER) plane_side(); else row_side();
        vd_lds_barrier();
        if constexpr (GATHER) row_side(); else plane_side();
        vd_lds_barrier();
    }
}

// A workgroup owns ONE stretch.  Scatter: an empty or SPARSE stretch (at most kVdSparse present cells) is written straight away --
// packs of fill, patched element by element where sidx names a row (none in an empty stretch: the fill streams); the others go
// through the tile.  Gather: every stretch with a present cell goes through vd_stretch.
// (Four consecutive stretches per workgroup, their index entries fetched at once, were measured: the 704 x 800 x 40 fill 5 % faster,
// the 88 x 100 x 5 map -- 172 stretches a sample -- twice as slow for the lost parallelism.  Not kept.)
// grid = out (scatter) or dense (gather): [n, c, p].
template <typename U, int VR, int VP, bool GATHER>
__global__ __launch_bounds__(kVdThreads) void k_vdense(U *__restrict__ rows, const int32_t *__restrict__ index, int32_t c, int64_t p,
                                                       int64_t stretches, U fill, U *__restrict__ grid)
{
    constexpr int SPC = kVdTile / VP;                          // packs of a plane's stretch
    typedef RowPack<U, VP> PP;
    __shared__ int32_t sidx[kVdTile];
    __shared__ int swave[kVdThreads / kWave];
    const int t = threadIdx.x;
    const int64_t sample = blockIdx.x / stretches, cell0 = (blockIdx.x % stretches) * kVdTile;
    const int live = (int)(p - cell0 < kVdTile ? p - cell0 : kVdTile);                      // cells of this stretch
    const int32_t mine = t < live ? index[sample * p + cell0 + t] : -1;
    sidx[t] = mine;
    const unsigned long long vote = __ballot(mine >= 0);
    if ((t & (kWave - 1)) == 0) swave[t / kWave] = __popcll(vote);
    vd_lds_barrier();
    int present = 0;
#pragma unroll
    for (int w = 0; w < kVdThreads / kWave; w++) present += swave[w];
    U *const planes = grid + sample * c * p + cell0;                                       // + ch * p + cell

    if (GATHER ? present == 0 : present <= kVdSparse) {
        if constexpr (!GATHER) {
            for (int64_t i = t; i < (int64_t)c * SPC; i += kVdThreads) {
                const int64_t ch = i / SPC;
                const int cell = (int)(i % SPC) * VP;
                if (cell >= live) continue;
                PP f;
#pragma unroll
                for (int q = 0; q < VP; q++) {
                    f.v[q] = fill;
                    if (present) {
                        const int32_t id = sidx[cell + q];
                        if (id >= 0) f.v[q] = rows[(int64_t)id * c + ch];
                    }
                }
                *(PP *)(planes + ch * p + cell) = f;
            }
        }
        return;
    }
    vd_stretch<U, VR, VP, GATHER>(rows, sidx, present, c, p, live, fill, planes);
}

// One lane per voxel: range test, flat cell, claim.  shape / origin: per DENSE axis (already permuted); col: the coordinate column
// each dense axis walks.
struct VdGeom {
    int64_t size[3], origin[3];
    int32_t col[3];
};
__global__ __launch_bounds__(kVdThreads) void k_vdense_map(const int64_t *__restrict__ coords, const int64_t *__restrict__ batch, int64_t v,
                                                           VdGeom geo, int64_t n, int64_t *__restrict__ cell, int32_t *__restrict__ index,
                                                           unsigned long long *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * kVdThreads + threadIdx.x;
    if (i >= v) return;
    const uint64_t b = batch ? (uint64_t)batch[i] : 0ull;
    bool inside = b < (uint64_t)n;
    uint64_t flat = b;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        // (uint64) coord - (uint64) origin < (uint64) size: no int64 value of either overflows the test
        const uint64_t rel = (uint64_t)coords[i * 3 + geo.col[a]] - (uint64_t)geo.origin[a];
        inside &= rel < (uint64_t)geo.size[a];
        flat = flat * (uint64_t)geo.size[a] + rel;
    }
    if (!inside) {
        cell[i] = -1;
        atomicAdd(&counts[0], 1ull);
        return;
    }
    cell[i] = (int64_t)flat;
    if (atomicCAS((int *)&index[flat], -1, (int)i) != -1) atomicAdd(&counts[1], 1ull);
}

// fill -> the bits of `fill` rounded (to nearest even, once) to the dtype
uint64_t vd_fill_bits(double fill, int32_t dtype)
{
    union { double d; uint64_t u; } d64 = {fill};
    if (dtype == D3D_F64) return d64.u;
    if (dtype == D3D_F16) {
        union { _Float16 h; uint16_t u; } h16 = {(_Float16)fill};
        return h16.u;
    }
    union { float f; uint32_t u; } f32 = {(float)fill};
    if (dtype == D3D_F32) return f32.u;
    // bf16: fp32 rounded TO ODD first (truncate, then set the last bit of an inexact value), so that the second rounding sees what
    // the first one dropped
    if (fill != fill) return 0x7fc0u;
    if ((double)f32.f != fill) {
        if (((double)f32.f < 0 ? -(double)f32.f : (double)f32.f) > (fill < 0 ? -fill : fill)) f32.u -= 1;
        f32.u |= 1u;
    }
    return (f32.u + 0x7fffu + ((f32.u >> 16) & 1u)) >> 16;
}

bool vd_dtype_ok(int32_t dtype) { return dtype == D3D_F32 || dtype == D3D_F64 || dtype == D3D_F16 || dtype == D3D_BF16; }

// the one launch site of k_vdense: element size -> U, the two VEC rules (row_dispatch's: 16 bytes where the extent is a multiple of
// 16 / s and the base is 16-byte aligned) -> VR, VP
template <bool GATHER>
int vd_launch(const char *name, const void *rows, const int32_t *index, int64_t n, int32_t c, int64_t p, int32_t dtype, uint64_t fill,
              const void *grid, hipStream_t st)
{
    const int64_t stretches = d3d_divup(p, kVdTile);
    if (n * stretches > kVdMaxStretches) return D3D_ERR_UNSUPPORTED;
    const int s = dtype == D3D_F64 ? 8 : dtype == D3D_F32 ? 4 : 2;
    return dispatch_int<2, 4, 8>(s, [&](auto ss) {
        typedef typename VdWord<decltype(ss)::value>::type U;
        constexpr int W = 16 / (int)sizeof(U);
        return dispatch(c % W == 0 && row_aligned16(rows), [&](auto wr) {
            return dispatch(p % W == 0 && row_aligned16(grid), [&](auto wp) {
                D3D_LAUNCH(name, (k_vdense<U, decltype(wr)::value ? W : 1, decltype(wp)::value ? W : 1, GATHER>), 
                           dim3((unsigned)(n * stretches)), dim3(kVdThreads), 0, st, (U *)rows, index, c, p, stretches, (U)fill, (U *)grid);
                return D3D_OK;
            });
        });
    });
}

}  // namespace

extern "C" int32_t d3d_vdense_tile_cells(void) { return kVdTile; }
extern "C" int32_t d3d_vdense_sparse_cells(void) { return kVdSparse; }

extern "C" int d3d_vdense_map(const int64_t *coords, const int64_t *batch, int64_t v, const int64_t *shape, const int64_t *origin,
                              const int32_t *axes, int64_t batch_size, int64_t *cell, int32_t *index, int64_t *counts, void *stream)
{
    if (v < 0 || batch_size < 1 || !shape || !origin || !axes || !counts) return D3D_ERR_BAD_ARG;
    bool seen[3] = {false, false, false};
    VdGeom geo;
    int64_t cells = batch_size;
    for (int a = 0; a < 3; a++) {
        const int32_t col = axes[a];
        if (col < 0 || col > 2 || seen[col] || shape[col] < 1) return D3D_ERR_BAD_ARG;
        seen[col] = true;
        geo.col[a] = col, geo.size[a] = shape[col], geo.origin[a] = origin[col];
        if (shape[col] > (kVdMaxStretches * kVdTile) / cells) return D3D_ERR_UNSUPPORTED;
        cells *= shape[col];
    }
    if (v > kRowMax) return D3D_ERR_UNSUPPORTED;
    if (!index || (v > 0 && (!coords || !cell))) return D3D_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    D3D_HIP_CHECK(hipMemsetAsync(index, 0xff, (size_t)cells * sizeof(int32_t), st));
    D3D_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    if (v == 0) return D3D_OK;
    D3D_LAUNCH("k_vdense_map", k_vdense_map, dim3((unsigned)d3d_divup(v, kVdThreads)), dim3(kVdThreads), 0, st, coords, batch, v, geo, batch_size,
               cell, index, (unsigned long long *)counts);
    return D3D_OK;
}

extern "C" int d3d_vdense_scatter(const void *feat, int64_t v, int32_t c, int32_t dtype, const int32_t *index, int64_t n,
                                  int64_t cells_per_sample, double fill, void *out, void *stream)
{
    if (v < 0 || c < 0 || n < 0 || cells_per_sample < 0) return D3D_ERR_BAD_ARG;
    if (!vd_dtype_ok(dtype) || v > kRowMax) return D3D_ERR_UNSUPPORTED;
    if (c == 0 || n == 0 || cells_per_sample == 0) return D3D_OK;
    if (!index || !out || (v > 0 && !feat)) return D3D_ERR_BAD_ARG;
    return vd_launch<false>("k_vdense<scatter>", feat, index, n, c, cells_per_sample, dtype, vd_fill_bits(fill, dtype), out, (hipStream_t)stream);
}

extern "C" int d3d_vdense_gather(const void *dense, int64_t n, int32_t c, int32_t dtype, const int32_t *index, int64_t cells_per_sample,
                                 int64_t v, void *out, void *stream)
{
    if (v < 0 || c < 0 || n < 0 || cells_per_sample < 0) return D3D_ERR_BAD_ARG;
    if (!vd_dtype_ok(dtype) || v > kRowMax) return D3D_ERR_UNSUPPORTED;
    if (c == 0 || v == 0 || n == 0 || cells_per_sample == 0) return D3D_OK;
    if (!index || !out || !dense) return D3D_ERR_BAD_ARG;
    return vd_launch<true>("k_vdense<gather>", out, index, n, c, cells_per_sample, dtype, 0, dense, (hipStream_t)stream);
}
