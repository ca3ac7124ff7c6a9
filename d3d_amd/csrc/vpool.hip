// vpool.hip -- per-voxel pooling of per-point feature rows on MI355X (gfx950): features[K,C] -> out[V,C] by sum / mean / max /
// min over the points of each voxel, and the gather back (voxel -> its points) that is both its gradient and voxel_unpool.  An
// extension: the reference reduces the raw input columns inside its voxelizer only (voxelize.cpp:137-164), without a gradient.
//
// No float atomics anywhere.  The mapping (voxel id per point, -1 = none) is inverted ONCE into a CSR index
//   order[K']    the mapped points grouped by ascending voxel id, ascending point index inside a voxel
//   offsets[V+1] where each voxel's slice of `order` starts
// (k_vi_keys: integer histogram + sort keys; the scan trio of common.hpp: offsets; sort.hip's stable argsort on V-1-id: order),
// and every pooling call walks it: one lane GROUP per voxel, a lane per 16 bytes of the row, the voxel's rows folded STRICTLY in
// point order -- the sum is the left fold np.add.at computes, the same bits on every run and for every launch shape.  A crowded
// voxel is a long sequential fold by contract: splitting it into partial sums would change the bits.  The rows' addresses do not
// depend on the fold, so four rows are in flight per step.  The backward pass / unpool is a gather, one lane group per point
// row: every output row is written exactly once (a zero row for a point without a voxel), nothing is zeroed beforehand.
#include <algorithm>
#include "vrow.hpp"

namespace {

constexpr int kPoolThreads = 256;
constexpr int kPoolAhead = 4;                 // rows in flight per lane and step of the fold

// ---------------------------------------------------------------- the index
// keys[i] = V - 1 - id for a mapped point (the argsort is DESCENDING and keeps ties in index order), -1 otherwise: after the
// mapped ones.  hist[id]++ (integer atomics: the result does not depend on the arrival order); ids outside [-1, V) are counted,
// one atomic per wavefront that saw any.
__global__ __launch_bounds__(kPoolThreads) void k_vi_keys(const int64_t *__restrict__ mapping, int64_t k, int64_t v,
                                                          int32_t *__restrict__ keys, uint32_t *__restrict__ hist,
                                                          int64_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x;
    bool bad = false;
    if (i < k) {
        const int64_t m = mapping[i];
        const bool ok = m >= 0 && m < v;
        keys[i] = ok ? (int32_t)(v - 1 - m) : -1;
        if (ok) atomicAdd(&hist[m], 1u);
        bad = !ok && m != -1;
    }
    const unsigned long long b = __ballot(bad);
    if (b && (threadIdx.x & (kWave - 1)) == 0) atomicAdd((unsigned long long *)&counts[1], (unsigned long long)__popcll(b));
}

// offsets[i] = points of the voxels before voxel i, i = 0 .. V (item V adds nothing: offsets[V] = K')
struct VoxelOffsets {
    static constexpr const char *kName = "k_scan_count<VoxelOffsets>", *kName2 = "k_scan_apply<VoxelOffsets>";
    const uint32_t *hist;
    int64_t v;
    int64_t *offsets;
    __device__ unsigned long long value(int64_t i) const { return i < v ? hist[i] : 0u; }
    __device__ unsigned long long value2(int64_t i) const { return value(i); }
    __device__ void apply(int64_t i, unsigned long long, unsigned long long excl) const { offsets[i] = (int64_t)excl; }
};

struct IndexWs {
    uint32_t *hist;
    int32_t *keys;
    unsigned long long *bsum;
    void *sort;
    size_t sort_bytes;
};
// the one layout: carved here for d3d_voxel_index, and on a null base for the size query
IndexWs index_carve(WsCarver &w, int64_t k, int64_t v)
{
    IndexWs r;
    r.hist = w.take<uint32_t>((size_t)v + 1);
    r.keys = w.take<int32_t>((size_t)std::max<int64_t>(k, 1));
    r.bsum = w.take<unsigned long long>((size_t)d3d_divup(v + 1, kScanTile));
    r.sort_bytes = d3d_internal_argsort_i32_bytes(k);
    r.sort = w.take<char>(r.sort_bytes);
    return r;
}

// ---------------------------------------------------------------- forward
// One lane group (1 << group_log2 lanes) per voxel, lane g of it on the VEC channels from g * VEC, then from
// (g + group) * VEC, ... (a C the group does not cover in one pass).  The rows are folded in point order by row_fold (vrow.hpp:
// max / min name the winning point).  Empty voxel: 0, arg -1.
template <typename T, int VEC, int RED, bool ARG>
__global__ __launch_bounds__(kPoolThreads) void k_vpool_fwd(const T *__restrict__ feat, const int32_t *__restrict__ order,
                                                            const int64_t *__restrict__ offsets, int64_t v, int32_t c, int group_log2,
                                                            T *__restrict__ out, int32_t *__restrict__ arg)
{
    typedef RowPack<T, VEC> P;
    const int64_t t = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x, vox = t >> group_log2;
    if (vox >= v) return;
    const int g = (int)(t & ((1 << group_log2) - 1)), step = VEC << group_log2;
    const int64_t beg = offsets[vox], end = offsets[vox + 1];
    for (int c0 = g * VEC; c0 < c; c0 += step) {
        T acc[VEC];
        int32_t win[VEC];
#pragma unroll
        for (int q = 0; q < VEC; q++) { acc[q] = 0; win[q] = -1; }
        auto fold = [&](const P &x, int32_t p) { row_fold<RED>(acc, win, x, p); };
        int64_t j = beg;
        for (; j + kPoolAhead <= end; j += kPoolAhead) {
            int32_t p[kPoolAhead];
            P x[kPoolAhead];
#pragma unroll
            for (int a = 0; a < kPoolAhead; a++) p[a] = order[j + a];
#pragma unroll
            for (int a = 0; a < kPoolAhead; a++) x[a] = *(const P *)(feat + (int64_t)p[a] * c + c0);
#pragma unroll
            for (int a = 0; a < kPoolAhead; a++) fold(x[a], p[a]);
        }
        for (; j < end; j++) {
            const int32_t p = order[j];
            fold(*(const P *)(feat + (int64_t)p * c + c0), p);
        }
        P o;
#pragma unroll
        for (int q = 0; q < VEC; q++) o.v[q] = (RED == D3D_REDUCE_MEAN && end > beg) ? acc[q] / (T)(end - beg) : acc[q];
        *(P *)(out + vox * c + c0) = o;
        if constexpr (ARG) {
            RowPack<int32_t, VEC> w;
#pragma unroll
            for (int q = 0; q < VEC; q++) w.v[q] = win[q];
            *(RowPack<int32_t, VEC> *)(arg + vox * c + c0) = w;
        }
    }
}

// ---------------------------------------------------------------- backward / unpool
// One lane group per point row i: grad_feat[i] = grad_out[m] (SUM), / (T)count[m] (MEAN), where arg[m] == i (MAX / MIN); a zero
// row for m outside [0, V).
template <typename T, int VEC, int RED>
__global__ __launch_bounds__(kPoolThreads) void k_vpool_bwd(const T *__restrict__ grad_out, const int64_t *__restrict__ mapping,
                                                            const int64_t *__restrict__ offsets, const int32_t *__restrict__ arg,
                                                            int64_t k, int64_t v, int32_t c, int group_log2, T *__restrict__ grad_feat)
{
    typedef RowPack<T, VEC> P;
    const int64_t t = (int64_t)blockIdx.x * kPoolThreads + threadIdx.x, i = t >> group_log2;
    if (i >= k) return;
    const int g = (int)(t & ((1 << group_log2) - 1)), step = VEC << group_log2;
    const int64_t m = mapping[i];
    const bool ok = m >= 0 && m < v;
    T cnt = 1;
    if constexpr (RED == D3D_REDUCE_MEAN) {
        if (ok) cnt = (T)(offsets[m + 1] - offsets[m]);
    }
    for (int c0 = g * VEC; c0 < c; c0 += step) {
        P o;
#pragma unroll
        for (int q = 0; q < VEC; q++) o.v[q] = 0;
        if (ok) {
            const P gv = *(const P *)(grad_out + m * c + c0);
            if constexpr (RED == D3D_REDUCE_MAX || RED == D3D_REDUCE_MIN) {
                const RowPack<int32_t, VEC> w = *(const RowPack<int32_t, VEC> *)(arg + m * c + c0);
#pragma unroll
                for (int q = 0; q < VEC; q++) o.v[q] = (int64_t)w.v[q] == i ? gv.v[q] : (T)0;
            } else {
#pragma unroll
                for (int q = 0; q < VEC; q++) o.v[q] = RED == D3D_REDUCE_MEAN ? gv.v[q] / cnt : gv.v[q];
            }
        }
        *(P *)(grad_feat + i * c + c0) = o;
    }
}

}  // namespace

extern "C" size_t d3d_voxel_index_workspace_bytes(int64_t k, int64_t v)
{
    WsCarver w(nullptr, 0);
    index_carve(w, std::max<int64_t>(k, 0), std::max<int64_t>(v, 0));
    return w.off;
}

extern "C" int d3d_voxel_index(const int64_t *mapping, int64_t k, int64_t v, int32_t *order, int64_t *offsets, int64_t *counts,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (k < 0 || v < 0 || !offsets || !counts || (k > 0 && (!mapping || !order))) return D3D_ERR_BAD_ARG;
    if (k > kRowMax || v > kRowMax) return D3D_ERR_UNSUPPORTED;
    WsCarver w(workspace, workspace_bytes);
    const IndexWs ws = index_carve(w, k, v);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    D3D_HIP_CHECK(hipMemsetAsync(ws.hist, 0, ((size_t)v + 1) * sizeof(uint32_t), st));
    D3D_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    if (k > 0)
        D3D_LAUNCH("k_vi_keys", k_vi_keys, dim3((unsigned)d3d_divup(k, kPoolThreads)), dim3(kPoolThreads), 0, st, mapping, k, v, ws.keys,
                   ws.hist, counts);
    const VoxelOffsets f{ws.hist, v, offsets};
    if (const int rc = d3d_run_scan(f, v + 1, ws.bsum, counts, -1, 0, 0ull, st); rc != D3D_OK) return rc;
    if (k > 0 && v > 0) return d3d_internal_argsort_desc_i32(ws.keys, k, order, ws.sort, ws.sort_bytes, st);
    return D3D_OK;
}

extern "C" int d3d_voxel_pool_forward(const void *feat, int64_t k, int32_t c, int32_t dtype, const int32_t *order, const int64_t *offsets,
                                      int64_t v, int32_t reduction, void *out, int32_t *arg, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (k < 0 || v < 0 || c < 1) return D3D_ERR_BAD_ARG;
    if (!row_reduction_ok(reduction) || (dtype != D3D_F32 && dtype != D3D_F64) || k > kRowMax || v > kRowMax) return D3D_ERR_UNSUPPORTED;
    if (v == 0) return D3D_OK;
    if (!out || !offsets || (k > 0 && (!feat || !order))) return D3D_ERR_BAD_ARG;
    const bool extreme = reduction == D3D_REDUCE_MAX || reduction == D3D_REDUCE_MIN;
    if (!extreme) arg = nullptr;                 // (there is no winner to name)
    const bool aligned = row_aligned16(feat) && row_aligned16(out) && row_aligned16(arg);
    return row_dispatch<D3D_F32, D3D_F64>(dtype, c, aligned, reduction, [&](auto p, auto vec, auto red, int gl) {
        typedef typename decltype(p)::T T;
        constexpr int VEC = decltype(vec)::value, RED = decltype(red)::value;
        return dispatch(arg != nullptr, [&](auto a) {
            constexpr bool ARG = decltype(a)::value && (RED == D3D_REDUCE_MAX || RED == D3D_REDUCE_MIN);
            D3D_LAUNCH(ARG ? "k_vpool_fwd<arg>" : "k_vpool_fwd", (k_vpool_fwd<T, VEC, RED, ARG>), dim3((unsigned)d3d_divup(v << gl, kPoolThreads)),
                       dim3(kPoolThreads), 0, st, (const T *)feat, order, offsets, v, c, gl, (T *)out, arg);
            return D3D_OK;
        });
    });
}

extern "C" int d3d_voxel_pool_backward(const void *grad_out, int64_t v, int32_t c, int32_t dtype, const int64_t *mapping, int64_t k,
                                       const int64_t *offsets, int32_t reduction, const int32_t *arg, void *grad_feat, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (k < 0 || v < 0 || c < 1) return D3D_ERR_BAD_ARG;
    if (!row_reduction_ok(reduction) || (dtype != D3D_F32 && dtype != D3D_F64) || k > kRowMax || v > kRowMax) return D3D_ERR_UNSUPPORTED;
    if (k == 0) return D3D_OK;
    const bool extreme = reduction == D3D_REDUCE_MAX || reduction == D3D_REDUCE_MIN;
    if (!grad_feat || !mapping || (v > 0 && (!grad_out || (extreme && !arg) || (reduction == D3D_REDUCE_MEAN && !offsets))))
        return D3D_ERR_BAD_ARG;
    const bool aligned = row_aligned16(grad_out) && row_aligned16(grad_feat) && (!extreme || row_aligned16(arg));
    return row_dispatch<D3D_F32, D3D_F64>(dtype, c, aligned, reduction, [&](auto p, auto vec, auto red, int gl) {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH("k_vpool_bwd", (k_vpool_bwd<T, decltype(vec)::value, decltype(red)::value>), dim3((unsigned)d3d_divup(k << gl, kPoolThreads)),
                   dim3(kPoolThreads), 0, st, (const T *)grad_out, mapping, offsets, arg, k, v, c, gl, (T *)grad_feat);
        return D3D_OK;
    });
}
