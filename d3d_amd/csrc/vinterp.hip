// vinterp.hip -- trilinear (or nearest) interpolation of sparse voxel features at arbitrary points and its transpose, the splat of
// point rows onto the voxels, on MI355X (gfx950): the devoxelize step of SPVCNN / PVCNN, PV-RCNN's keypoint features, the point head
// of a sparse U-Net, in fp32, fp64, fp16 and bf16.  An extension: the reference stops at the voxelizer.  The corner table and its
// weights come from d3d_voxel_corners (vnbr.hip).
//
//   d3d_table_interp_forward   feat[V, C], table[R, J], weights[R, J]            -> out[R, C]       = sum_j w[r, j] feat[table[r, j]]
//   d3d_table_interp_backward  grad[R, C], order, offsets, weights[R * J]        -> grad_feat[V, C] = sum_e w[e] grad[e / J]
//   d3d_knn_interp_forward / _backward: the same two for a table of ANY width 1 .. D3D_KNN_MAX (a kNN or ball-query table with its
//     weights: three_interpolate and its gradient) -- the same kernel through InterpRowsAny / SplatRowsAny, J a run-time value
//
// Both are ONE kernel, k_wfold: a weighted fold of source rows, one launch, no workspace, no read-back, no float atomics.  What differs
// is where an output row finds its entries (InterpRows: the J entries of its table row; SplatRows: its slice of the inverted index
// d3d_voxel_index made of the flattened table) -- so the splat's forward is the interpolation's backward and the other way round.
// An output row is 0, then + w * x per PRESENT entry in ascending entry order, the product and the sum two separate roundings (the
// build does not contract); an absent corner (-1) is skipped, not a zero row.  Strictly in that order: the same bits on every run, a
// row's bits depend on its own entries only -- not on its position, the launch shape or the path (vector or scalar).  Half types:
// products and sums in fp32 (RowAcc), one rounding (to nearest even) at the store.
//
// One lane GROUP (a power of two, at most a wavefront) per output row, a lane per 16 bytes of it (per element on the scalar path).
// Per step of the fold every lane reads the step's entries and weights first (the same addresses across the group: one fetch), then
// starts the loads of all the present rows, then folds them: J = 8 rows in flight for the interpolation (the whole table row), four
// for the splat, whose folds are as long as their voxel is crowded -- a long sequential fold by contract, as in vpool.hip: that
// launch lasts as long as its most crowded voxel's fold.  (Eight rows per step and the next step's entries fetched under this
// step's rows were measured once on a frame whose most crowded voxel has 1350 entries: 0.49 against 0.51 ms, not kept.)
//
// Bytes moved (s = the element size, w = the weight size: 8 for fp64, 4 otherwise; E = the present entries):
//   forward   R J (4 + w) of table and weights + R C s stored; the E C s of gathered rows hit the caches wherever neighbouring points
//             share corners (a V C s read is the floor)
//   backward  8 (V + 1) of offsets + E (4 + w) of order and weights + E C s of gathered gradient rows (neighbouring entries of a voxel
//             name neighbouring points' rows only where the points are sorted in space) + V C s stored
#include <type_traits>
#include "vrow.hpp"

namespace {

constexpr int kWfThreads = 256;
constexpr int kWfSplatAhead = 4;              // rows in flight per lane and step of a voxel's fold

// where output row r finds its entries: [beg, end) in steps of kAhead; entry i -> its number e in the flattened table (weights[e])
// and the source row it names, -1 for none
template <int J> struct InterpRows {          // row r of table[R, J]: entries r J .. r J + J - 1, each names feat[table[e]]
    static constexpr int kAhead = J;
    const int32_t *table;
    __device__ void range(int64_t r, int64_t &beg, int64_t &end) const { beg = r * J, end = beg + J; }
    __device__ void entry(int64_t i, int64_t &e, int64_t &src) const { e = i, src = table[i]; }
};
template <int J> struct SplatRows {           // voxel v: order[offsets[v] .. offsets[v + 1]), entry e names grad[e / J]
    static constexpr int kAhead = kWfSplatAhead;
    const int32_t *order;
    const int64_t *offsets;
    __device__ void range(int64_t r, int64_t &beg, int64_t &end) const { beg = offsets[r], end = offsets[r + 1]; }
    __device__ void entry(int64_t i, int64_t &e, int64_t &src) const { e = order[i], src = e / J; }
};
// their siblings with the width taken at run time (d3d_knn_interp_*: any j in 1 .. D3D_KNN_MAX), four rows in flight
struct InterpRowsAny {
    static constexpr int kAhead = kWfSplatAhead;
    const int32_t *table;
    int32_t j;
    __device__ void range(int64_t r, int64_t &beg, int64_t &end) const { beg = r * j, end = beg + j; }
    __device__ void entry(int64_t i, int64_t &e, int64_t &src) const { e = i, src = table[i]; }
};
struct SplatRowsAny {
    static constexpr int kAhead = kWfSplatAhead;
    const int32_t *order;
    const int64_t *offsets;
    int32_t j;
    __device__ void range(int64_t r, int64_t &beg, int64_t &end) const { beg = offsets[r], end = offsets[r + 1]; }
    __device__ void entry(int64_t i, int64_t &e, int64_t &src) const { e = order[i], src = e / j; }
};

// Lane g of the group on the VEC channels from g * VEC, then from (g + group) * VEC, ... (a C the group does not cover in one pass;
// the entries are walked once per pass).  A row without present entries: 0.
template <typename T, int VEC, class Rows>
__global__ __launch_bounds__(kWfThreads) void k_wfold(const T *__restrict__ src, Rows rows, const typename RowAcc<T>::type *__restrict__ weights,
                                                      int64_t n, int32_t c, int gl, T *__restrict__ out)
{
    typedef RowPack<T, VEC> P;
    typedef typename RowAcc<T>::type A;
    constexpr int AH = Rows::kAhead;
    const int64_t t = (int64_t)blockIdx.x * kWfThreads + threadIdx.x, r = t >> gl;
    if (r >= n) return;
    const int g = (int)(t & ((1 << gl) - 1)), step = VEC << gl;
    int64_t beg, end;
    rows.range(r, beg, end);
    for (int c0 = g * VEC; c0 < c; c0 += step) {
        A acc[VEC];
#pragma unroll
        for (int q = 0; q < VEC; q++) acc[q] = 0;
        for (int64_t i = beg; i < end; i += AH) {
            int64_t s[AH];
            A w[AH];
            P x[AH];
#pragma unroll
            for (int a = 0; a < AH; a++) {
                s[a] = -1, w[a] = 0;
                if (i + a < end) {
                    int64_t e;
                    rows.entry(i + a, e, s[a]);
                    w[a] = weights[e];
                }
            }
#pragma unroll
            for (int a = 0; a < AH; a++)
                if (s[a] >= 0) x[a] = *(const P *)(src + s[a] * c + c0);
#pragma unroll
            for (int a = 0; a < AH; a++)
                if (s[a] >= 0) {
#pragma unroll
                    for (int q = 0; q < VEC; q++) {
                        const A prod = w[a] * (A)x[a].v[q];
                        acc[q] = acc[q] + prod;
                    }
                }
        }
        P o;
#pragma unroll
        for (int q = 0; q < VEC; q++) o.v[q] = (T)acc[q];
        *(P *)(out + r * c + c0) = o;
    }
}

// what the entries refuse: D3D_OK to go on.  any_width: j in 1 .. D3D_KNN_MAX (the d3d_knn_interp_* entries) instead of 1 or 8
int wf_check(int64_t src_rows, int64_t rows, int64_t v, int32_t c, int32_t dtype, int32_t j, bool any_width = false)
{
    if (src_rows < 0 || rows < 0 || v < 0 || c < 1 || (any_width ? j < 1 : (j != 1 && j != 8))) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64 && dtype != D3D_F16 && dtype != D3D_BF16) return D3D_ERR_UNSUPPORTED;
    if (j > D3D_KNN_MAX || v > kRowMax || rows > kRowMax / j) return D3D_ERR_UNSUPPORTED;
    return D3D_OK;
}

// the one launch site: `n` output rows of c channels in `dtype`, their entries by `rows` (one of the four Rows structs)
template <class Rows>
int wf_launch(const char *name, const void *src, const void *weights, int64_t n, int32_t c, int32_t dtype, void *out, hipStream_t st,
              const Rows &rows)
{
    return row_dispatch<D3D_F32, D3D_F64, D3D_F16, D3D_BF16>(dtype, c, row_aligned16(src) && row_aligned16(out), [&](auto p, auto vec, int gl) {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH(name, (k_wfold<T, decltype(vec)::value, Rows>), dim3((unsigned)d3d_divup(n << gl, kWfThreads)), dim3(kWfThreads), 0, st,
                   (const T *)src, rows, (const typename RowAcc<T>::type *)weights, n, c, gl, (T *)out);
        return D3D_OK;
    });
}

}  // namespace

extern "C" int d3d_table_interp_forward(const void *feat, int64_t v, int32_t c, int32_t dtype, const int32_t *table, const void *weights,
                                        int64_t rows, int32_t j, void *out, void *stream)
{
    if (const int rc = wf_check(v, rows, v, c, dtype, j); rc != D3D_OK) return rc;
    if (rows == 0) return D3D_OK;
    if (!table || !weights || !out || (v > 0 && !feat)) return D3D_ERR_BAD_ARG;
    return dispatch_int<1, 8>(j, [&](auto jj) {
        return wf_launch("k_wfold<interp>", feat, weights, rows, c, dtype, out, (hipStream_t)stream, InterpRows<decltype(jj)::value>{table});
    });
}

extern "C" int d3d_table_interp_backward(const void *grad, int64_t rows, int32_t c, int32_t dtype, const int32_t *order, const int64_t *offsets,
                                         const void *weights, int32_t j, int64_t v, void *grad_feat, void *stream)
{
    if (const int rc = wf_check(rows, rows, v, c, dtype, j); rc != D3D_OK) return rc;
    if (v == 0) return D3D_OK;
    if (!offsets || !grad_feat || (rows > 0 && (!grad || !order || !weights))) return D3D_ERR_BAD_ARG;
    return dispatch_int<1, 8>(j, [&](auto jj) {
        return wf_launch("k_wfold<splat>", grad, weights, v, c, dtype, grad_feat, (hipStream_t)stream,
                         SplatRows<decltype(jj)::value>{order, offsets});
    });
}

extern "C" int d3d_knn_interp_forward(const void *feat, int64_t v, int32_t c, int32_t dtype, const int32_t *table, const void *weights,
                                      int64_t rows, int32_t j, void *out, void *stream)
{
    if (const int rc = wf_check(v, rows, v, c, dtype, j, true); rc != D3D_OK) return rc;
    if (rows == 0) return D3D_OK;
    if (!table || !weights || !out || (v > 0 && !feat)) return D3D_ERR_BAD_ARG;
    return wf_launch("k_wfold<knn interp>", feat, weights, rows, c, dtype, out, (hipStream_t)stream, InterpRowsAny{table, j});
}

extern "C" int d3d_knn_interp_backward(const void *grad, int64_t rows, int32_t c, int32_t dtype, const int32_t *order, const int64_t *offsets,
                                       const void *weights, int32_t j, int64_t v, void *grad_feat, void *stream)
{
    if (const int rc = wf_check(rows, rows, v, c, dtype, j, true); rc != D3D_OK) return rc;
    if (v == 0) return D3D_OK;
    if (!offsets || !grad_feat || (rows > 0 && (!grad || !order || !weights))) return D3D_ERR_BAD_ARG;
    return wf_launch("k_wfold<knn splat>", grad, weights, v, c, dtype, grad_feat, (hipStream_t)stream, SplatRowsAny{order, offsets, j});
}
