// vtpool.hip -- pooling through the tables of the sparse convolutions on MI355X (gfx950): sum / mean / max / min over the rows a table
// row names (spconv's SparseMaxPool3d / SparseAvgPool3d), in fp32, fp64, fp16 and bf16, and its gradient.  An extension: the
// reference stops at the voxelizer.
//
//   d3d_table_pool_forward   feat[src_rows, C], table[rows, K]            -> out[rows, C] (+ arg[rows, C] int16, count[rows])
//   d3d_table_pool_backward  grad_out[out_rows, C], back_table[rows, K]   -> grad_feat[rows, C]
//   d3d_table_pool_backward_index  grad_out[rows, C], order, offsets      -> grad_feat[src_rows, C]   (a table without a transposed table)
//
// Both are a reduce-while-gathering, one launch each, no workspace, no float atomics: the tables are each other's transposed map
// (table_out[r, k] == v <=> table_in[v, k] == r; a VoxelNeighbors' table against its own mirrored columns), so the gradient of "row r
// reduces the rows its table row names" is "row v adds up what the rows of ITS table row owe it" -- again a gather, every output row
// written exactly once.  An absent entry (-1) is skipped, it is not a zero row: the [rows, K, C] buffer of d3d_neighbor_gather, its
// mask and its K-fold traffic never exist.
//
// One lane GROUP (a power of two, at most a wavefront) per output row, a lane per 16 bytes of it (per element on the scalar path).
// The group reads its table row in pieces of up to four entries per lane (coalesced), ballots turn each piece into the bit mask of
// its present entries, and the lanes walk the set bits in ascending column order, the entry broadcast by a shuffle inside the group:
// the loop runs over the PRESENT entries only, up to four row loads in flight per lane.  The fold is strictly in ascending column,
// so a row's bits depend on its table row and the rows it names alone -- not on its position, the launch shape, the path (vector or
// scalar) or the run.  Half types: sums in fp32, one rounding (to nearest even) at the store; max / min are exact in every type.
#include <algorithm>
#include "vrow.hpp"

namespace {

constexpr int kTpThreads = 256;
constexpr int kTpAhead = 4;                   // rows in flight per lane and step of the walk
constexpr int kTpEntries = 4;                 // table entries per lane and piece of the table row (tp_walk selects among exactly 4)
constexpr int kTpMaxK = 343;                  // 7^3: arg is int16

// The walk of one table row by its lane group (lane g of 1 << gl, the group's first lane of the wavefront lane0): load(e, a)
// starts the loads of entry e into slot a, fold(kk, a) folds slot a as column kk; per step up to kTpAhead loads, then their folds,
// ascending in kk.  A piece of the row is up to kTpEntries entries per lane (entry i of it in register i >> gl of lane i & (G - 1),
// at most 64 per piece: the mask of the present ones is one word), so that a narrow group does not pay one dependent table load
// per two or four entries.  Every lane of the group must be here (the entries come from the group's lanes); -> the present entries.
template <class Load, class Fold>
__device__ __forceinline__ int tp_walk(const int32_t *__restrict__ trow, int K, int g, int gl, int lane0, Load &&load, Fold &&fold)
{
    const int G = 1 << gl, E = std::min(kTpEntries, kWave >> gl);
    const unsigned long long gmask = G == kWave ? ~0ull : ((1ull << G) - 1ull);
    int n = 0;
    for (int base = 0; base < K; base += E << gl) {
        int32_t e[kTpEntries];
        unsigned long long m = 0;                                            // (the same in every lane of the group)
#pragma unroll
        for (int j = 0; j < kTpEntries; j++) {
            const int kk = base + (j << gl) + g;
            e[j] = (j < E && kk < K) ? trow[kk] : -1;
        }
#pragma unroll
        for (int j = 0; j < kTpEntries; j++)
            if (j < E) m |= ((__ballot(e[j] >= 0) >> lane0) & gmask) << (j << gl);
        n += __popcll(m);
        while (m) {
            int i[kTpAhead];
#pragma unroll
            for (int a = 0; a < kTpAhead; a++) {
                i[a] = m ? __ffsll((long long)m) - 1 : -1;
                m &= m - 1;
            }
#pragma unroll
            for (int a = 0; a < kTpAhead; a++) {
                const int idx = i[a] < 0 ? 0 : i[a], j = idx >> gl;
                const int32_t mine = j == 0 ? e[0] : j == 1 ? e[1] : j == 2 ? e[2] : e[3];
                const int32_t ea = __shfl(mine, idx & (G - 1), G);
                if (i[a] >= 0) load(ea, a);
            }
#pragma unroll
            for (int a = 0; a < kTpAhead; a++)
                if (i[a] >= 0) fold(base + i[a], a);
        }
    }
    return n;
}

// ---------------------------------------------------------------- forward
// Lane g of the group on the VEC channels from g * VEC, then from (g + group) * VEC, ... (a C the group does not cover in one
// pass; the table row is walked once per pass).  The rows are folded in ascending column by row_fold (vrow.hpp: max / min name
// the winning column).  A row without entries: 0, arg -1, count 0.
template <typename T, int VEC, int RED, bool ARG>
__global__ __launch_bounds__(kTpThreads) void k_tpool_fwd(const T *__restrict__ feat, const int32_t *__restrict__ table, int64_t rows,
                                                          int32_t K, int32_t c, int gl, T *__restrict__ out, int16_t *__restrict__ arg,
                                                          int32_t *__restrict__ count)
{
    typedef RowPack<T, VEC> P;
    typedef typename RowAcc<T>::type A;
    const int64_t t = (int64_t)blockIdx.x * kTpThreads + threadIdx.x, r = t >> gl;
    if (r >= rows) return;                                                   // (whole groups leave: a row never spans two of them)
    const int g = (int)(t & ((1 << gl) - 1)), step = VEC << gl, lane0 = (int)(threadIdx.x & (kWave - 1)) & ~((1 << gl) - 1);
    const int32_t *trow = table + r * K;
    for (int cb = 0; cb < c; cb += step) {
        const int c0 = cb + g * VEC;
        const bool live = c0 < c;                                            // (a group wider than the row: its last lanes only share entries)
        A acc[VEC];                                                          // (the sum, or the best so far: a half value as the fp32 it is)
        int32_t win[VEC];
        P x[kTpAhead];
#pragma unroll
        for (int q = 0; q < VEC; q++) { acc[q] = 0; win[q] = -1; }
#pragma unroll
        for (int a = 0; a < kTpAhead; a++)
#pragma unroll
            for (int q = 0; q < VEC; q++) x[a].v[q] = 0;
        const int n = tp_walk(trow, K, g, gl, lane0,
            [&](int32_t e, int a) { if (live) x[a] = *(const P *)(feat + (int64_t)e * c + c0); },
            [&](int kk, int a) { row_fold<RED>(acc, win, x[a], kk); });
        if (count && cb == 0 && g == 0) count[r] = n;
        if (!live) continue;
        P o;
#pragma unroll
        for (int q = 0; q < VEC; q++) o.v[q] = (T)((RED == D3D_REDUCE_MEAN && n > 0) ? acc[q] / (A)n : acc[q]);
        *(P *)(out + r * c + c0) = o;
        if constexpr (ARG) {
            RowPack<int16_t, VEC> w;
#pragma unroll
            for (int q = 0; q < VEC; q++) w.v[q] = (int16_t)win[q];
            *(RowPack<int16_t, VEC> *)(arg + r * c + c0) = w;
        }
    }
}

// ---------------------------------------------------------------- backward
// Row v of back_table: entry e of column kk reached v through column fk = mirrored ? K - 1 - kk : kk of the forward, and owes it
// grad_out[e] (SUM), grad_out[e] / (T)count[e] (MEAN), grad_out[e, ch] where arg[e, ch] == fk (MAX / MIN); summed from 0 in
// ascending kk.
template <typename T, int VEC, int RED>
__global__ __launch_bounds__(kTpThreads) void k_tpool_bwd(const T *__restrict__ grad_out, const int32_t *__restrict__ back, int64_t rows,
                                                          int32_t K, int32_t c, int32_t mirrored, int gl, const int16_t *__restrict__ arg,
                                                          const int32_t *__restrict__ count, T *__restrict__ grad_feat)
{
    typedef RowPack<T, VEC> P;
    typedef RowPack<int16_t, VEC> W;
    typedef typename RowAcc<T>::type A;
    constexpr bool EXTREME = RED == D3D_REDUCE_MAX || RED == D3D_REDUCE_MIN;
    const int64_t t = (int64_t)blockIdx.x * kTpThreads + threadIdx.x, r = t >> gl;
    if (r >= rows) return;
    const int g = (int)(t & ((1 << gl) - 1)), step = VEC << gl, lane0 = (int)(threadIdx.x & (kWave - 1)) & ~((1 << gl) - 1);
    const int32_t *trow = back + r * K;
    for (int cb = 0; cb < c; cb += step) {
        const int c0 = cb + g * VEC;
        const bool live = c0 < c;
        A acc[VEC];
        P x[kTpAhead];
        W w[kTpAhead];
        A cnt[kTpAhead];
#pragma unroll
        for (int q = 0; q < VEC; q++) acc[q] = 0;
#pragma unroll
        for (int a = 0; a < kTpAhead; a++) {
            cnt[a] = 1;
#pragma unroll
            for (int q = 0; q < VEC; q++) { x[a].v[q] = 0; w[a].v[q] = -1; }
        }
        tp_walk(trow, K, g, gl, lane0,
            [&](int32_t e, int a) {
                if (!live) return;
                x[a] = *(const P *)(grad_out + (int64_t)e * c + c0);
                if constexpr (EXTREME) w[a] = *(const W *)(arg + (int64_t)e * c + c0);
                if constexpr (RED == D3D_REDUCE_MEAN) cnt[a] = (A)count[e];
            },
            [&](int kk, int a) {
                const int fk = mirrored ? K - 1 - kk : kk;
#pragma unroll
                for (int q = 0; q < VEC; q++) {
                    if constexpr (EXTREME) acc[q] = (int)w[a].v[q] == fk ? acc[q] + (A)x[a].v[q] : acc[q];
                    else if constexpr (RED == D3D_REDUCE_MEAN) acc[q] += (A)x[a].v[q] / cnt[a];
                    else acc[q] += (A)x[a].v[q];
                }
            });
        if (!live) continue;
        P o;
#pragma unroll
        for (int q = 0; q < VEC; q++) o.v[q] = (T)acc[q];
        *(P *)(grad_feat + r * c + c0) = o;
    }
}

// ---------------------------------------------------------------- backward through an inverted index
// For a table that has no fixed-width transposed table -- the cells of RoIs, a ball-query or kNN table: a source row is named by as
// many entries as boxes overlap it.  Source row v walks order[offsets[v] .. offsets[v + 1]), the entries e = r * K + kk that hold v in
// ascending e (d3d_knn_interp_backward's layout), four in flight, and adds what each owes it by k_tpool_bwd's rules.  No ballots:
// the lanes of a group only share the row.
constexpr int kTpIndexAhead = 4;
template <typename T, int VEC, int RED>
__global__ __launch_bounds__(kTpThreads) void k_tpool_bwd_index(const T *__restrict__ grad_out, const int32_t *__restrict__ order,
                                                                const int64_t *__restrict__ offsets, int64_t src_rows, int32_t K, int32_t c,
                                                                int gl, const int16_t *__restrict__ arg, const int32_t *__restrict__ count,
                                                                T *__restrict__ grad_feat)
{
    typedef RowPack<T, VEC> P;
    typedef RowPack<int16_t, VEC> W;
    typedef typename RowAcc<T>::type A;
    constexpr bool EXTREME = RED == D3D_REDUCE_MAX || RED == D3D_REDUCE_MIN;
    constexpr int AH = kTpIndexAhead;
    const int64_t t = (int64_t)blockIdx.x * kTpThreads + threadIdx.x, v = t >> gl;
    if (v >= src_rows) return;
    const int g = (int)(t & ((1 << gl) - 1)), step = VEC << gl;
    const int64_t beg = offsets[v], end = offsets[v + 1];
    for (int c0 = g * VEC; c0 < c; c0 += step) {
        A acc[VEC];
#pragma unroll
        for (int q = 0; q < VEC; q++) acc[q] = 0;
        for (int64_t i = beg; i < end; i += AH) {
            int64_t r[AH];
            int kk[AH];
            P x[AH];
            W w[AH];
            A cnt[AH];
#pragma unroll
            for (int a = 0; a < AH; a++) {
                r[a] = -1, kk[a] = 0, cnt[a] = 1;
                if (i + a < end) {
                    const int32_t e = order[i + a];
                    r[a] = e / K, kk[a] = e - (int32_t)r[a] * K;
                }
            }
#pragma unroll
            for (int a = 0; a < AH; a++)
                if (r[a] >= 0) {
                    x[a] = *(const P *)(grad_out + r[a] * c + c0);
                    if constexpr (EXTREME) w[a] = *(const W *)(arg + r[a] * c + c0);
                    if constexpr (RED == D3D_REDUCE_MEAN) cnt[a] = (A)count[r[a]];
                }
#pragma unroll
            for (int a = 0; a < AH; a++)
                if (r[a] >= 0) {
#pragma unroll
                    for (int q = 0; q < VEC; q++) {
                        if constexpr (EXTREME) acc[q] = (int)w[a].v[q] == kk[a] ? acc[q] + (A)x[a].v[q] : acc[q];
                        else if constexpr (RED == D3D_REDUCE_MEAN) acc[q] += (A)x[a].v[q] / cnt[a];
                        else acc[q] += (A)x[a].v[q];
                    }
                }
        }
        P o;
#pragma unroll
        for (int q = 0; q < VEC; q++) o.v[q] = (T)acc[q];
        *(P *)(grad_feat + v * c + c0) = o;
    }
}

bool tp_dtype_ok(int32_t d) { return d == D3D_F32 || d == D3D_F64 || d == D3D_F16 || d == D3D_BF16; }

}  // namespace

extern "C" int d3d_table_pool_forward(const void *feat, int64_t src_rows, int32_t c, int32_t dtype, const int32_t *table, int64_t rows,
                                      int32_t k, int32_t reduction, void *out, int16_t *arg, int32_t *count, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (src_rows < 0 || rows < 0 || c < 1 || k < 1) return D3D_ERR_BAD_ARG;
    if (!row_reduction_ok(reduction) || !tp_dtype_ok(dtype) || k > kTpMaxK || rows > kRowMax || src_rows > kRowMax) return D3D_ERR_UNSUPPORTED;
    if (rows == 0) return D3D_OK;
    if (!table || !out || (src_rows > 0 && !feat)) return D3D_ERR_BAD_ARG;
    const bool extreme = reduction == D3D_REDUCE_MAX || reduction == D3D_REDUCE_MIN;
    if (!extreme) arg = nullptr;                 // (there is no winner to name)
    const bool aligned = row_aligned16(feat) && row_aligned16(out) && row_aligned16(arg);
    return row_dispatch<D3D_F32, D3D_F64, D3D_F16, D3D_BF16>(dtype, c, aligned, reduction, [&](auto p, auto vec, auto red, int gl) {
        typedef typename decltype(p)::T T;
        constexpr int VEC = decltype(vec)::value, RED = decltype(red)::value;
        return dispatch(arg != nullptr, [&](auto a) {
            constexpr bool ARG = decltype(a)::value && (RED == D3D_REDUCE_MAX || RED == D3D_REDUCE_MIN);
            D3D_LAUNCH(ARG ? "k_tpool_fwd<arg>" : "k_tpool_fwd", (k_tpool_fwd<T, VEC, RED, ARG>), dim3((unsigned)d3d_divup(rows << gl, kTpThreads)),
                       dim3(kTpThreads), 0, st, (const T *)feat, table, rows, k, c, gl, (T *)out, arg, count);
            return D3D_OK;
        });
    });
}

extern "C" int d3d_table_pool_backward(const void *grad_out, int64_t out_rows, int32_t c, int32_t dtype, const int32_t *back_table,
                                       int64_t rows, int32_t k, int32_t mirrored, int32_t reduction, const int16_t *arg,
                                       const int32_t *count, void *grad_feat, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (out_rows < 0 || rows < 0 || c < 1 || k < 1) return D3D_ERR_BAD_ARG;
    if (!row_reduction_ok(reduction) || !tp_dtype_ok(dtype) || k > kTpMaxK || rows > kRowMax || out_rows > kRowMax) return D3D_ERR_UNSUPPORTED;
    if (rows == 0) return D3D_OK;
    const bool extreme = reduction == D3D_REDUCE_MAX || reduction == D3D_REDUCE_MIN;
    if (!back_table || !grad_feat || (out_rows > 0 && (!grad_out || (extreme && !arg) || (reduction == D3D_REDUCE_MEAN && !count))))
        return D3D_ERR_BAD_ARG;
    const bool aligned = row_aligned16(grad_out) && row_aligned16(grad_feat) && (!extreme || row_aligned16(arg));
    return row_dispatch<D3D_F32, D3D_F64, D3D_F16, D3D_BF16>(dtype, c, aligned, reduction, [&](auto p, auto vec, auto red, int gl) {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH("k_tpool_bwd", (k_tpool_bwd<T, decltype(vec)::value, decltype(red)::value>), dim3((unsigned)d3d_divup(rows << gl, kTpThreads)),
                   dim3(kTpThreads), 0, st, (const T *)grad_out, back_table, rows, k, c, mirrored, gl, arg, count, (T *)grad_feat);
        return D3D_OK;
    });
}

extern "C" int d3d_table_pool_backward_index(const void *grad_out, int64_t rows, int32_t c, int32_t dtype, const int32_t *order,
                                             const int64_t *offsets, int64_t src_rows, int32_t k, int32_t reduction, const int16_t *arg,
                                             const int32_t *count, void *grad_feat, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (rows < 0 || src_rows < 0 || c < 1 || k < 1) return D3D_ERR_BAD_ARG;
    if (!row_reduction_ok(reduction) || !tp_dtype_ok(dtype) || k > kTpMaxK || src_rows > kRowMax || rows > kRowMax / k) return D3D_ERR_UNSUPPORTED;
    if (src_rows == 0) return D3D_OK;
    const bool extreme = reduction == D3D_REDUCE_MAX || reduction == D3D_REDUCE_MIN;
    if (!offsets || !grad_feat || (rows > 0 && (!grad_out || !order || (extreme && !arg) || (reduction == D3D_REDUCE_MEAN && !count))))
        return D3D_ERR_BAD_ARG;
    const bool aligned = row_aligned16(grad_out) && row_aligned16(grad_feat) && (!extreme || row_aligned16(arg));
    return row_dispatch<D3D_F32, D3D_F64, D3D_F16, D3D_BF16>(dtype, c, aligned, reduction, [&](auto p, auto vec, auto red, int gl) {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH("k_tpool_bwd_index", (k_tpool_bwd_index<T, decltype(vec)::value, decltype(red)::value>),
                   dim3((unsigned)d3d_divup(src_rows << gl, kTpThreads)), dim3(kTpThreads), 0, st, (const T *)grad_out, order, offsets, src_rows,
                   k, c, gl, arg, count, (T *)grad_feat);
        return D3D_OK;
    });
}
