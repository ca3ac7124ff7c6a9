// vlift.hip -- the "lift, splat" view transform of LSS / BEVDet / BEVDepth / BEVFusion (bev_pool) on MI355X (gfx950): every pixel of
// every camera carries a depth distribution over D bins and a context row of C channels; the S D H W frustum points are placed in
// the ego grid and each cell gets the sum of depth[p] * feat[pixel(p)] over its points.  The result lands as voxel rows [V, C] with
// coords, the currency of the rest of the voxel stack.  An extension: the reference has no counterpart.
//
//   d3d_frustum_map_count / _emit   us, vs, ds, pre[S, 3, 4], post[S, 3, 4], the grid  -> mapping[K], coords[V, 3], batch_index[V]
//   d3d_lift_pool_forward           depth[S, D, H, W], feat[S, H, W, C], order, offsets -> out[V, C]
//   d3d_lift_pool_backward_feat     grad[V, C], depth, mapping                          -> grad_feat[S, H, W, C]
//   d3d_lift_pool_backward_depth    grad[V, C], feat, mapping                           -> grad_depth[S, D, H, W]
//
// The map: one lane per frustum point computes its cell in fp32, one rounding per operation (the build does not contract), marks
// the cell in a bitmap (integer atomics: the result does not depend on the arrival order) and keeps the cell's key; the scan trio
// of common.hpp numbers the marked cells by ascending key, so the numbering is a function of the input alone; _emit turns keys into
// rows and decodes the present keys into coords.  Every dependency is a kernel boundary, nothing waits on another workgroup.  The
// inverted index (order, offsets) is d3d_voxel_index's, unchanged.
//
// The folds: no float atomics, one launch each, no workspace, no read-back; the [K, C] product never exists.  Forward: one lane
// GROUP per voxel row, a lane per 16 bytes of it, the row's points folded STRICTLY in `order` (vpool.hip's shape, with eight feature
// rows in flight per step and the next step's entries of `order` fetched under them; a crowded near-camera cell is a long sequential
// fold by contract, and the launch lasts as long as the most crowded cell's lane group needs: its instruction stream and one trip to
// memory per step, which is why the pixel of an entry is found by a multiplication, not a division).  backward_feat is a gather:
// one lane group per pixel, its D points folded in ascending d, consecutive groups on consecutive w so a wavefront's mapping /
// depth reads run along w.  backward_depth: one lane group per point, the channel products reduced across the group.
#include <algorithm>
#include <cmath>
#include "vrow.hpp"

namespace {

constexpr int kLiftThreads = 256;
constexpr int kLiftAhead = 8;                 // rows in flight per lane and step of the forward fold (4: 0.125 / 0.055 ms where 8 takes 0.102 / 0.049)
constexpr int kLiftBins = 4;                  // depth bins in flight per lane and step of backward_feat (8: 0.133 ms where 4 takes 0.106)

// ---------------------------------------------------------------- the map
struct FmGrid {
    float lo[3], size[3];
    int32_t shape[3];
};

// Point i = ((s d_n + d) h_n + h) w_n + w -> cell[i] = its key ((b n0 + c0) n1 + c1) n2 + c2, or -1 for a point outside; a member
// sets bit (key & 31) of bitmap[key >> 5]; counts[1] += members, one atomic per wavefront that saw any.
__global__ __launch_bounds__(kLiftThreads) void k_fm_cells(const float *__restrict__ us, const float *__restrict__ vs,
                                                           const float *__restrict__ ds, const float *__restrict__ pre,
                                                           const float *__restrict__ post, FmGrid g, uint32_t wn, uint32_t hn, uint32_t dn,
                                                           int64_t k, uint32_t cams, int32_t *__restrict__ cell, uint32_t *__restrict__ bitmap,
                                                           int64_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * kLiftThreads + threadIdx.x;
    bool member = false;
    if (i < k) {
        uint32_t r = (uint32_t)i;
        const uint32_t iw = r % wn;
        r /= wn;
        const uint32_t ih = r % hn;
        r /= hn;
        const uint32_t id = r % dn, s = r / dn;
        const float a0 = us[iw], a1 = vs[ih], a2 = ds[id];
        const float *m = pre + (size_t)s * 12, *n = post + (size_t)s * 12;
        float q[3], x[3];
#pragma unroll
        for (int j = 0; j < 3; j++) q[j] = ((m[4 * j] * a0 + m[4 * j + 1] * a1) + m[4 * j + 2] * a2) + m[4 * j + 3];
        const float e0 = q[0] * q[2], e1 = q[1] * q[2], e2 = q[2];
#pragma unroll
        for (int j = 0; j < 3; j++) x[j] = ((n[4 * j] * e0 + n[4 * j + 1] * e1) + n[4 * j + 2] * e2) + n[4 * j + 3];
        member = true;
        int64_t key = s / cams;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float t = (x[j] - g.lo[j]) / g.size[j];
            // t < shape for a t >= 0 is (int) t < shape; NaN fails the first comparison, 2^31 and more the second
            const bool ok = t >= 0.0f && t < 2147483648.0f && (int32_t)t < g.shape[j];
            member &= ok;
            key = key * g.shape[j] + (ok ? (int32_t)t : 0);
        }
        cell[i] = member ? (int32_t)key : -1;
        if (member) atomicOr(&bitmap[key >> 5], 1u << (key & 31));
    }
    const unsigned long long b = __ballot(member);
    if (b && (threadIdx.x & (kWave - 1)) == 0) atomicAdd((unsigned long long *)&counts[1], (unsigned long long)__popcll(b));
}

// prefix[i] = the present cells in the words before word i; the total is V
struct CellWords {
    static constexpr const char *kName = "k_scan_count<CellWords>", *kName2 = "k_scan_apply<CellWords>";
    const uint32_t *bitmap;
    uint32_t *prefix;
    __device__ unsigned long long value(int64_t i) const { return (unsigned long long)__popc(bitmap[i]); }
    __device__ unsigned long long value2(int64_t i) const { return value(i); }
    __device__ void apply(int64_t i, unsigned long long, unsigned long long excl) const { prefix[i] = (uint32_t)excl; }
};

// mapping[i] = the row of point i's cell: the present cells below its key
__global__ __launch_bounds__(kLiftThreads) void k_fm_rows(const int32_t *__restrict__ cell, const uint32_t *__restrict__ bitmap,
                                                          const uint32_t *__restrict__ prefix, int64_t k, int64_t *__restrict__ mapping)
{
    const int64_t i = (int64_t)blockIdx.x * kLiftThreads + threadIdx.x;
    if (i >= k) return;
    const int32_t key = cell[i];
    int64_t row = -1;
    if (key >= 0) row = (int64_t)prefix[key >> 5] + __popc(bitmap[key >> 5] & ((1u << (key & 31)) - 1u));
    mapping[i] = row;
}

// one lane per word of the bitmap: its present cells, decoded, from row prefix[word] on (rows below v only: a v smaller than the
// count's is refused by the bound, not written past)
__global__ __launch_bounds__(kLiftThreads) void k_fm_coords(const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ prefix,
                                                            int64_t words, FmGrid g, int64_t v, int64_t *__restrict__ coords,
                                                            int64_t *__restrict__ batch_index)
{
    const int64_t i = (int64_t)blockIdx.x * kLiftThreads + threadIdx.x;
    if (i >= words) return;
    uint32_t word = bitmap[i];
    int64_t row = prefix[i];
    while (word && row < v) {
        const int bit = __ffs((int)word) - 1;
        word &= word - 1;
        int64_t key = i * 32 + bit;
        const int64_t c2 = key % g.shape[2];
        key /= g.shape[2];
        const int64_t c1 = key % g.shape[1];
        key /= g.shape[1];
        coords[row * 3 + 0] = key % g.shape[0];
        coords[row * 3 + 1] = c1;
        coords[row * 3 + 2] = c2;
        batch_index[row] = key / g.shape[0];
        row++;
    }
}

struct FmWs {
    int32_t *cell;
    uint32_t *bitmap, *prefix;
    unsigned long long *bsum;
};
// the one layout: carved here for the two entries, and on a null base for the size query
FmWs fm_carve(WsCarver &w, int64_t k, int64_t words)
{
    FmWs r;
    r.cell = w.take<int32_t>((size_t)std::max<int64_t>(k, 1));
    r.bitmap = w.take<uint32_t>((size_t)words);
    r.prefix = w.take<uint32_t>((size_t)words);
    r.bsum = w.take<unsigned long long>((size_t)d3d_divup(words, kScanTile));
    return r;
}

// the product of four sizes >= 0, saturated at kRowMax + 1 after every factor (no intermediate overflows; a later 0 still gives 0)
int64_t lift_product(int64_t a, int64_t b, int64_t c, int64_t d)
{
    __int128 p = 1;
    for (const int64_t f : {a, b, c, d}) p = std::min<__int128>(p * f, (__int128)kRowMax + 1);
    return (int64_t)p;
}

// the sizes of a map: D3D_OK and k = S D H W, cells = B n0 n1 n2, or the refusal.  BAD_ARG comes first, then UNSUPPORTED.
int fm_sizes(int32_t wn, int32_t hn, int32_t dn, int64_t s, int32_t cams, const int32_t *shape, int64_t &k, int64_t &cells)
{
    if (wn < 0 || hn < 0 || dn < 0 || s < 0 || cams < 1 || !shape || s % cams != 0) return D3D_ERR_BAD_ARG;
    if (shape[0] < 1 || shape[1] < 1 || shape[2] < 1) return D3D_ERR_BAD_ARG;
    k = lift_product(s, dn, hn, wn);
    cells = lift_product(std::max<int64_t>(s / cams, 1), shape[0], shape[1], shape[2]);
    if (k > kRowMax || cells > kRowMax) return D3D_ERR_UNSUPPORTED;
    return D3D_OK;
}

FmGrid fm_grid(const float *lo, const float *size, const int32_t *shape)
{
    FmGrid g;
    for (int j = 0; j < 3; j++) {
        g.lo[j] = lo ? lo[j] : 0.0f, g.size[j] = size ? size[j] : 1.0f, g.shape[j] = shape[j];
    }
    return g;
}

// ---------------------------------------------------------------- the folds
// n / d for n below 2^31 as a multiplication (Granlund & Montgomery: with l = ceil(log2 d) and m = ceil(2^(31 + l) / d) < 2^32,
// (n m) >> (31 + l) is the quotient for every n < 2^31): the folds take two quotients per ENTRY, and the instruction stream of the
// most crowded cell's lane group is what the forward launch waits for -- there is no integer divide instruction, a 32-bit division
// is some 40 instructions (k_lift_fwd: 0.157 -> 0.125 ms at BEVFusion's shape)
struct LiftDiv {
    uint32_t d, m, sh;
    __device__ __forceinline__ uint32_t operator()(uint32_t n) const { return (uint32_t)(((uint64_t)n * m) >> sh); }
};
LiftDiv lift_div(uint32_t d)
{
    d = std::max(d, 1u);
    uint32_t l = 0;
    while ((1ull << l) < d) l++;
    return LiftDiv{d, (uint32_t)(((1ull << (31 + l)) + d - 1) / d), 31 + l};
}
// pixel row of point p: its camera's plane, its (h, w) -- (p / (D H W)) H W + p % (H W)
__device__ __forceinline__ int64_t lift_pix(uint32_t p, const LiftDiv &dhw, const LiftDiv &hw)
{
    return (int64_t)(dhw(p) * hw.d + (p - hw(p) * hw.d));
}

// Forward.  Lane g of voxel row vox's group on the VEC channels from g * VEC, then from (g + group) * VEC, ...: 0, then
// + (depth[p] * feat[pix(p)]) over p in order[offsets[vox] .. offsets[vox + 1]) in that order, product and sum two roundings in A.
template <typename T, int VEC>
__global__ __launch_bounds__(kLiftThreads) void k_lift_fwd(const T *__restrict__ depth, const T *__restrict__ feat,
                                                           const int32_t *__restrict__ order, const int64_t *__restrict__ offsets, int64_t v,
                                                           LiftDiv dhw, LiftDiv hw, int32_t c, int gl, T *__restrict__ out)
{
    typedef RowPack<T, VEC> P;
    typedef typename RowAcc<T>::type A;
    const int64_t t = (int64_t)blockIdx.x * kLiftThreads + threadIdx.x, vox = t >> gl;
    if (vox >= v) return;
    const int g = (int)(t & ((1 << gl) - 1)), step = VEC << gl;
    const int64_t beg = offsets[vox], end = offsets[vox + 1];
    for (int c0 = g * VEC; c0 < c; c0 += step) {
        A acc[VEC];
#pragma unroll
        for (int q = 0; q < VEC; q++) acc[q] = 0;
        auto fold = [&](A w, const P &x) {
#pragma unroll
            for (int q = 0; q < VEC; q++) {
                const A prod = w * (A)x.v[q];
                acc[q] = acc[q] + prod;
            }
        };
        // a step's rows hang on its entries of `order`: the NEXT step's entries are fetched under this step's rows (on its own this
        // changed nothing measurable -- the entries of a step mostly share a cache line with the last step's; profiles/lift_profile.txt)
        uint32_t next[kLiftAhead];
        int64_t j = beg;
#pragma unroll
        for (int a = 0; a < kLiftAhead; a++) next[a] = j + a < end ? (uint32_t)order[j + a] : 0u;
        for (; j + kLiftAhead <= end; j += kLiftAhead) {
            uint32_t p[kLiftAhead];
            A w[kLiftAhead];
            P x[kLiftAhead];
#pragma unroll
            for (int a = 0; a < kLiftAhead; a++) {
                p[a] = next[a];
                w[a] = (A)depth[p[a]];
                x[a] = *(const P *)(feat + lift_pix(p[a], dhw, hw) * c + c0);
            }
#pragma unroll
            for (int a = 0; a < kLiftAhead; a++) next[a] = j + kLiftAhead + a < end ? (uint32_t)order[j + kLiftAhead + a] : 0u;
#pragma unroll
            for (int a = 0; a < kLiftAhead; a++) fold(w[a], x[a]);
        }
#pragma unroll
        for (int a = 0; a < kLiftAhead - 1; a++)
            if (j + a < end) fold((A)depth[next[a]], *(const P *)(feat + lift_pix(next[a], dhw, hw) * c + c0));
        P o;
#pragma unroll
        for (int q = 0; q < VEC; q++) o.v[q] = (T)acc[q];
        *(P *)(out + vox * c + c0) = o;
    }
}

// The gradient in feat, a gather.  One lane group per pixel (s, h, w): 0, then + (depth[p] * grad[mapping[p]]) over d ascending for
// the points p = (s D + d) H W + hw of the pixel that have a row.  Every row is written once.
template <typename T, int VEC>
__global__ __launch_bounds__(kLiftThreads) void k_lift_bwd_feat(const T *__restrict__ grad, const T *__restrict__ depth,
                                                                const int64_t *__restrict__ mapping, int64_t pixels, int64_t v, uint32_t dn,
                                                                uint32_t hw, int32_t c, int gl, T *__restrict__ grad_feat)
{
    typedef RowPack<T, VEC> P;
    typedef typename RowAcc<T>::type A;
    const int64_t t = (int64_t)blockIdx.x * kLiftThreads + threadIdx.x, pix = t >> gl;
    if (pix >= pixels) return;
    const int g = (int)(t & ((1 << gl) - 1)), step = VEC << gl;
    const int64_t first = (pix / hw) * dn * hw + pix % hw;        // the pixel's point at d = 0; d steps by hw
    for (int c0 = g * VEC; c0 < c; c0 += step) {
        A acc[VEC];
#pragma unroll
        for (int q = 0; q < VEC; q++) acc[q] = 0;
        // the rows and weights of the bins d0 .. d0 + kLiftBins - 1 (-1: no row, or no such bin)
        auto entries = [&](uint32_t d0, int64_t (&m)[kLiftBins], A (&w)[kLiftBins]) {
#pragma unroll
            for (int a = 0; a < kLiftBins; a++) {
                m[a] = -1, w[a] = 0;
                if (d0 + a < dn) {
                    const int64_t p = first + (int64_t)(d0 + a) * hw;
                    m[a] = mapping[p];
                    w[a] = (A)depth[p];
                    if (m[a] >= v) m[a] = -1;
                }
            }
        };
        // as in the forward: the next step's entries are fetched under this step's gradient rows
        int64_t mn[kLiftBins];
        A wn[kLiftBins];
        entries(0, mn, wn);
        for (uint32_t d0 = 0; d0 < dn; d0 += kLiftBins) {
            int64_t m[kLiftBins];
            A w[kLiftBins];
            P x[kLiftBins];
#pragma unroll
            for (int a = 0; a < kLiftBins; a++) {
                m[a] = mn[a], w[a] = wn[a];
                if (m[a] >= 0) x[a] = *(const P *)(grad + m[a] * c + c0);
            }
            entries(d0 + kLiftBins, mn, wn);
#pragma unroll
            for (int a = 0; a < kLiftBins; a++)
                if (m[a] >= 0) {
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
        *(P *)(grad_feat + pix * c + c0) = o;
    }
}

// The gradient in depth.  One lane group per point p: every lane sums (grad[m, ch] * feat[pix(p), ch]) over its channels in A, the
// group's sums are added pairwise (xor 1, 2, 4, ...), lane 0 of the group stores; 0 for a point without a row.  The order of the
// sum is this kernel's own: the one output of the operator that is not defined bit for bit.
template <typename T, int VEC>
__global__ __launch_bounds__(kLiftThreads) void k_lift_bwd_depth(const T *__restrict__ grad, const T *__restrict__ feat,
                                                                 const int64_t *__restrict__ mapping, int64_t k, int64_t v, LiftDiv dhw,
                                                                 LiftDiv hw, int32_t c, int gl, T *__restrict__ grad_depth)
{
    typedef RowPack<T, VEC> P;
    typedef typename RowAcc<T>::type A;
    const int64_t t = (int64_t)blockIdx.x * kLiftThreads + threadIdx.x, p = t >> gl;
    if (p >= k) return;                                            // (whole groups leave: a group never straddles k)
    const int g = (int)(t & ((1 << gl) - 1)), step = VEC << gl;
    const int64_t m = mapping[p];
    A acc = 0;
    if (m >= 0 && m < v) {
        const T *gr = grad + m * c, *fr = feat + lift_pix((uint32_t)p, dhw, hw) * c;
        for (int c0 = g * VEC; c0 < c; c0 += step) {
            const P x = *(const P *)(gr + c0), y = *(const P *)(fr + c0);
#pragma unroll
            for (int q = 0; q < VEC; q++) {
                const A prod = (A)x.v[q] * (A)y.v[q];
                acc = acc + prod;
            }
        }
    }
    for (int d = 1; d < (1 << gl); d <<= 1) acc = acc + __shfl_xor(acc, d, kWave);
    if (g == 0) grad_depth[p] = (T)acc;
}

// what the three folds refuse: D3D_OK to go on, with k = S D H W
int lift_check(int64_t s, int32_t dn, int32_t hn, int32_t wn, int32_t c, int32_t dtype, int64_t v, int64_t &k)
{
    if (s < 0 || dn < 0 || hn < 0 || wn < 0 || v < 0 || c < 1) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64 && dtype != D3D_F16 && dtype != D3D_BF16) return D3D_ERR_UNSUPPORTED;
    k = lift_product(s, dn, hn, wn);
    if (k > kRowMax || v > kRowMax) return D3D_ERR_UNSUPPORTED;
    return D3D_OK;
}

}  // namespace

extern "C" size_t d3d_frustum_map_workspace_bytes(int64_t k, int64_t cells)
{
    WsCarver w(nullptr, 0);
    fm_carve(w, std::max<int64_t>(k, 0), d3d_divup(std::max<int64_t>(cells, 1), 32));
    return w.off;
}

extern "C" int d3d_frustum_map_count(const float *us, int32_t wn, const float *vs, int32_t hn, const float *ds, int32_t dn, const float *pre,
                                     const float *post, int64_t s, int32_t cams_per_sample, const float *lo, const float *size,
                                     const int32_t *shape, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    int64_t k = 0, cells = 0;
    if (!lo || !size || !counts) return D3D_ERR_BAD_ARG;
    for (int j = 0; j < 3; j++)
        if (!(size[j] > 0.0f) || !std::isfinite(size[j])) return D3D_ERR_BAD_ARG;
    if (const int rc = fm_sizes(wn, hn, dn, s, cams_per_sample, shape, k, cells); rc != D3D_OK) return rc;
    if (k > 0 && (!us || !vs || !ds || !pre || !post)) return D3D_ERR_BAD_ARG;
    const int64_t words = d3d_divup(cells, 32);
    WsCarver w(workspace, workspace_bytes);
    const FmWs ws = fm_carve(w, k, words);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    const FmGrid g = fm_grid(lo, size, shape);
    D3D_HIP_CHECK(hipMemsetAsync(ws.bitmap, 0, (size_t)words * sizeof(uint32_t), st));
    D3D_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    if (k > 0)
        D3D_LAUNCH("k_fm_cells", k_fm_cells, dim3((unsigned)d3d_divup(k, kLiftThreads)), dim3(kLiftThreads), 0, st, us, vs, ds, pre, post, g,
                   (uint32_t)wn, (uint32_t)hn, (uint32_t)dn, k, (uint32_t)cams_per_sample, ws.cell, ws.bitmap, counts);
    const CellWords f{ws.bitmap, ws.prefix};
    return d3d_run_scan(f, words, ws.bsum, counts, -1, 0, 0ull, st);
}

extern "C" int d3d_frustum_map_emit(int32_t wn, int32_t hn, int32_t dn, int64_t s, int32_t cams_per_sample, const int32_t *shape, int64_t v,
                                    int64_t *mapping, int64_t *coords, int64_t *batch_index, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    int64_t k = 0, cells = 0;
    if (v < 0) return D3D_ERR_BAD_ARG;
    if (const int rc = fm_sizes(wn, hn, dn, s, cams_per_sample, shape, k, cells); rc != D3D_OK) return rc;
    if (v > cells) return D3D_ERR_BAD_ARG;
    if ((k > 0 && !mapping) || (v > 0 && (!coords || !batch_index))) return D3D_ERR_BAD_ARG;
    const int64_t words = d3d_divup(cells, 32);
    WsCarver w(workspace, workspace_bytes);
    const FmWs ws = fm_carve(w, k, words);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    if (k > 0)
        D3D_LAUNCH("k_fm_rows", k_fm_rows, dim3((unsigned)d3d_divup(k, kLiftThreads)), dim3(kLiftThreads), 0, st, ws.cell, ws.bitmap, ws.prefix,
                   k, mapping);
    if (v > 0)
        D3D_LAUNCH("k_fm_coords", k_fm_coords, dim3((unsigned)d3d_divup(words, kLiftThreads)), dim3(kLiftThreads), 0, st, ws.bitmap, ws.prefix,
                   words, fm_grid(nullptr, nullptr, shape), v, coords, batch_index);
    return D3D_OK;
}

extern "C" int d3d_lift_pool_forward(const void *depth, const void *feat, int64_t s, int32_t dn, int32_t hn, int32_t wn, int32_t c,
                                     int32_t dtype, const int32_t *order, const int64_t *offsets, int64_t v, void *out, void *stream)
{
    int64_t k = 0;
    if (const int rc = lift_check(s, dn, hn, wn, c, dtype, v, k); rc != D3D_OK) return rc;
    if (v == 0) return D3D_OK;
    if (!out || !offsets || (k > 0 && (!depth || !feat || !order))) return D3D_ERR_BAD_ARG;
    const LiftDiv hw = lift_div((uint32_t)hn * (uint32_t)wn), dhw = lift_div((uint32_t)hn * (uint32_t)wn * (uint32_t)dn);
    return row_dispatch<D3D_F32, D3D_F64, D3D_F16, D3D_BF16>(dtype, c, row_aligned16(feat) && row_aligned16(out), [&](auto p, auto vec, int gl) {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH("k_lift_fwd", (k_lift_fwd<T, decltype(vec)::value>), dim3((unsigned)d3d_divup(v << gl, kLiftThreads)), dim3(kLiftThreads), 0,
                   (hipStream_t)stream, (const T *)depth, (const T *)feat, order, offsets, v, dhw, hw, c, gl, (T *)out);
        return D3D_OK;
    });
}

extern "C" int d3d_lift_pool_backward_feat(const void *grad, int64_t v, const void *depth, const int64_t *mapping, int64_t s, int32_t dn,
                                           int32_t hn, int32_t wn, int32_t c, int32_t dtype, void *grad_feat, void *stream)
{
    int64_t k = 0;
    if (const int rc = lift_check(s, dn, hn, wn, c, dtype, v, k); rc != D3D_OK) return rc;
    const int64_t pixels = lift_product(s, hn, wn, 1);
    if (pixels > kRowMax) return D3D_ERR_UNSUPPORTED;                 // (dn == 0: k does not bound the pixels)
    if (pixels == 0) return D3D_OK;
    if (!grad_feat || (k > 0 && (!depth || !mapping)) || (k > 0 && v > 0 && !grad)) return D3D_ERR_BAD_ARG;
    const uint32_t hw = (uint32_t)hn * (uint32_t)wn;
    return row_dispatch<D3D_F32, D3D_F64, D3D_F16, D3D_BF16>(dtype, c, row_aligned16(grad) && row_aligned16(grad_feat),
                                                             [&](auto p, auto vec, int gl) {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH("k_lift_bwd_feat", (k_lift_bwd_feat<T, decltype(vec)::value>), dim3((unsigned)d3d_divup(pixels << gl, kLiftThreads)),
                   dim3(kLiftThreads), 0, (hipStream_t)stream, (const T *)grad, (const T *)depth, mapping, pixels, v, (uint32_t)dn, hw, c, gl,
                   (T *)grad_feat);
        return D3D_OK;
    });
}

extern "C" int d3d_lift_pool_backward_depth(const void *grad, int64_t v, const void *feat, const int64_t *mapping, int64_t s, int32_t dn,
                                            int32_t hn, int32_t wn, int32_t c, int32_t dtype, void *grad_depth, void *stream)
{
    int64_t k = 0;
    if (const int rc = lift_check(s, dn, hn, wn, c, dtype, v, k); rc != D3D_OK) return rc;
    if (k == 0) return D3D_OK;
    if (!grad_depth || !mapping || !feat || (v > 0 && !grad)) return D3D_ERR_BAD_ARG;
    const LiftDiv hw = lift_div((uint32_t)hn * (uint32_t)wn), dhw = lift_div((uint32_t)hn * (uint32_t)wn * (uint32_t)dn);
    return row_dispatch<D3D_F32, D3D_F64, D3D_F16, D3D_BF16>(dtype, c, row_aligned16(grad) && row_aligned16(feat), [&](auto p, auto vec, int gl) {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH("k_lift_bwd_depth", (k_lift_bwd_depth<T, decltype(vec)::value>), dim3((unsigned)d3d_divup(k << gl, kLiftThreads)),
                   dim3(kLiftThreads), 0, (hipStream_t)stream, (const T *)grad, (const T *)feat, mapping, k, v, dhw, hw, c, gl, (T *)grad_depth);
        return D3D_OK;
    });
}
