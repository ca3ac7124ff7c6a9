// boxsparse.hip -- the SPARSE box operators on MI355X (gfx950): of the [n,m] matrix of box2d_iou / iou3d only the entries above a
// threshold, as an ordered list (i, j, value) with CSR offsets, and never the matrix.  An extension: the reference offers the
// matrices only (d3d/box/iou.h:7-69, d3d/dgal_wrap.h:45-91), and at the densities of a driving scene fewer than 0.02 % of the
// pairs overlap at all -- the matrix of 100 k x 100 k boxes is 80 GB of zeros around a list of a few MB.
//
// The size of the list is known to the device only, so the entry comes in two passes over the same sweep:
//   d3d_iou_sparse_count   k_sp_aabb (the conservative fp32 bounding box of every boxes2 row, float4[m] in the workspace), k_sp_sweep
//                          <count> (hits per row), then three scan launches that turn the counts into offsets[n + 1] -- the scan
//                          shape of camera.hip: sums per tile, one workgroup over the sums, a scan inside every tile; no launch
//                          waits on another workgroup;
//   d3d_iou_sparse_emit    k_sp_aabb and k_sp_sweep<emit>: the same hits again -- the same expressions on the same values give the
//                          same bits -- stored at offsets[i] + rank.  Nothing sized by the number of candidates lives between the
//                          passes, and nothing is sorted: the price is that a candidate is clipped twice.
// The sweep: a workgroup of 4 wavefronts owns 4 x kSpRows rows and walks ALL columns in chunks of kSpChunk bounding boxes staged in
// LDS (each 16-byte box is fetched once per workgroup, not once per row); a wavefront tests 64 columns at a time against its rows
// (aabb_gap: two packed subtractions and three minima per pair), compacts the survivors by ballot into its LDS queue -- ascending
// columns stay ascending -- and only when 64 are queued does every lane take one pair through the per-pair functions of geom.hpp,
// the recipe of k_iou_paired / k_iou3d_paired (boxpair.hip), so a value is the matrix's value bit for bit.  The ~500 instructions
// of the clip thus run on full wavefronts, never on the one lane in 5000 that has a candidate.  The rank of a hit inside its row
// is a prefix popcount over the ballot of the hits of that row, on top of the row's running count: the queue holds the pairs of
// one row in ascending column order, whatever rows they are interleaved with.
// No spatial broad phase: every pair of bounding boxes is tested.
#include "common.hpp"
#include "geom.hpp"
#include <math.h>

namespace {

constexpr int kSpThreads = 256, kSpWaves = kSpThreads / kWave;
constexpr int kSpRows = 4;            // rows per wavefront: their bounding boxes stay in registers across the whole sweep
constexpr int kSpChunk = 1024;        // column bounding boxes staged per step (16 KiB of LDS)
constexpr int kSpQueue = 2 * kWave;   // per wavefront: fewer than 64 waiting plus up to 64 new
constexpr int kSpTile = 1024;         // rows per workgroup of the scan launches (4 per thread)

// row -> its values widened to the arithmetic's type and its BEV geometry, as k_iou_paired (5 columns: x, y, w, h, r) and
// k_iou3d_paired (7 columns: x, y, z, lx, ly, lz, rz) build them
template <typename TIn, typename T, int COLS>
__device__ __forceinline__ BoxGeom<T> load_geom(const TIn *__restrict__ row, T (&r)[COLS])
{
#pragma unroll
    for (int k = 0; k < COLS; k++) r[k] = (T)row[k];
    if constexpr (COLS == 5) return make_geom<T>(r[0], r[1], r[2], r[3], r[4]);
    else return make_geom<T>(r[0], r[1], r[3], r[4], r[6]);
}

__device__ __forceinline__ float4 empty_aabb() { return make_float4(INFINITY, INFINITY, -INFINITY, -INFINITY); }

template <typename TIn, typename T, int COLS, bool ROTATED>
__global__ __launch_bounds__(kSpThreads) void k_sp_aabb(const TIn *__restrict__ b2, int64_t m, float4 *__restrict__ cb)
{
    const int64_t j = (int64_t)blockIdx.x * kSpThreads + threadIdx.x;
    if (j >= m) return;
    T r[COLS];
    cb[j] = cand_aabb(load_geom<TIn, T, COLS>(b2 + j * COLS, r), ROTATED);
}

// EMIT = false: offsets[i] = the number of hits of row i (i < n).  EMIT = true: offsets[] are the scanned offsets; pairs / values
// are written, capacity rows of them exist.  thr: the threshold rounded to the stored type.
template <typename TIn, typename T, int COLS, bool ROTATED, bool EMIT>
__global__ __launch_bounds__(kSpThreads) void k_sp_sweep(const TIn *__restrict__ b1, int64_t n, const TIn *__restrict__ b2, int64_t m,
                                                         const float4 *__restrict__ cb, TIn thr, int64_t *__restrict__ offsets,
                                                         int64_t *__restrict__ pairs, TIn *__restrict__ values, int64_t capacity)
{
    __shared__ float4 scol[kSpChunk];
    __shared__ BoxGeom<T> srow[kSpWaves][kSpRows];
    __shared__ T szr[kSpWaves][kSpRows][2];                        // (zmax, zmin) of the rows, 7 columns only
    __shared__ unsigned long long squeue[kSpWaves][kSpQueue];      // (row slot : 32 | column : 32)
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t row0 = ((int64_t)blockIdx.x * kSpWaves + w) * kSpRows;
    // lane r of the wavefront builds row r; a slot past n keeps an empty bounding box and never has a candidate
    float4 mine = empty_aabb();
    if (lane < kSpRows && row0 + lane < n) {
        T r[COLS];
        const BoxGeom<T> g = load_geom<TIn, T, COLS>(b1 + (row0 + lane) * COLS, r);
        srow[w][lane] = g;
        if constexpr (COLS == 7) { szr[w][lane][0] = r[2] + r[5] / 2; szr[w][lane][1] = r[2] - r[5] / 2; }
        mine = cand_aabb(g, ROTATED);
    }
    float4 rbb[kSpRows];
    unsigned int cnt[kSpRows];                                      // hits of the row so far (wave-uniform)
#pragma unroll
    for (int r = 0; r < kSpRows; r++) {
        rbb[r] = make_float4(__shfl(mine.x, r, kWave), __shfl(mine.y, r, kWave), __shfl(mine.z, r, kWave), __shfl(mine.w, r, kWave));
        cnt[r] = 0;
    }
    unsigned long long *q = squeue[w];
    unsigned int wn = 0;                                            // wave-uniform fill of the queue

    // the first min(wn, 64) queued pairs, one per lane; what is behind them moves to the front
    auto clip = [&]() {
        __builtin_amdgcn_wave_barrier();          // LDS ops of one wavefront complete in order: no s_barrier needed
        const bool live = (unsigned int)lane < wn;
        int slot = -1;
        int64_t j = 0;
        TIn stored = 0;
        bool hit = false;
        if (live) {
            const unsigned long long e = q[lane];
            slot = (int)(e >> 32);
            j = (int64_t)(e & 0xffffffffull);
            const BoxGeom<T> a = srow[w][slot];
            T rb[COLS];
            const BoxGeom<T> b = load_geom<TIn, T, COLS>(b2 + j * COLS, rb);
            // (the pair is queued because aabb_gap(cand_aabb(a), cand_aabb(b)) > 0 on these very values: the test of the recipe)
            T v = ROTATED ? iou_rbox(a, b) : iou_aabb(a, b);
            if constexpr (COLS == 7) {
                const T azmax = szr[w][slot][0], azmin = szr[w][slot][1], bzmax = rb[2] + rb[5] / 2, bzmin = rb[2] - rb[5] / 2;
                const T imax = fmin(azmax, bzmax), imin = fmax(azmin, bzmin), umax = fmax(azmax, bzmax), umin = fmin(azmin, bzmin);
                const T zi = fmax(imax - imin, (T)0), zu = fmax(umax - umin, (T)1e-6);
                const T bev = v;
                v = 0;
                if (bev != 0) v = bev * (zi / zu);
            }
            stored = (TIn)v;
            hit = stored > thr;                    // strict, on the stored value; false for NaN
        }
        unsigned int rank = 0;
#pragma unroll
        for (int r = 0; r < kSpRows; r++) {
            const unsigned long long hits = __ballot(hit && slot == r);
            if (slot == r) rank = cnt[r] + (unsigned int)__popcll(hits & below);
            cnt[r] += (unsigned int)__popcll(hits);
        }
        if constexpr (EMIT) {
            if (hit) {
                const int64_t at = offsets[row0 + slot] + (int64_t)rank;
                if (at >= 0 && at < capacity) {        // (always, with the offsets of the count pass: foreign offsets must not write outside)
                    pairs[2 * at] = row0 + slot;
                    pairs[2 * at + 1] = j;
                    values[at] = stored;
                }
            }
        }
        const bool tail = (unsigned int)lane + kWave < wn;
        const unsigned long long moved = tail ? q[lane + kWave] : 0ull;
        __builtin_amdgcn_wave_barrier();
        if (tail) q[lane] = moved;
        wn = wn > (unsigned int)kWave ? wn - kWave : 0u;
    };

    for (int64_t c0 = 0; c0 < m; c0 += kSpChunk) {
        __syncthreads();                                            // the previous chunk has been read by everybody
        for (int t = threadIdx.x; t < kSpChunk; t += kSpThreads) scol[t] = c0 + t < m ? cb[c0 + t] : empty_aabb();
        __syncthreads();
        const int cols = (int)(m - c0 < kSpChunk ? m - c0 : kSpChunk);
        for (int s0 = 0; s0 < cols; s0 += kWave) {
            const float4 bb = scol[s0 + lane];
            float g[kSpRows], best = -1.f;
#pragma unroll
            for (int r = 0; r < kSpRows; r++) { g[r] = aabb_gap(rbb[r], bb); best = fmaxf(best, g[r]); }
            if (__ballot(best > 0.f) == 0) continue;                // (almost always)
#pragma unroll
            for (int r = 0; r < kSpRows; r++) {
                const bool cand = g[r] > 0.f;
                const unsigned long long mask = __ballot(cand);
                if (mask == 0) continue;
                if (cand) q[wn + (unsigned int)__popcll(mask & below)] = ((unsigned long long)r << 32) | (unsigned long long)(c0 + s0 + lane);
                wn += (unsigned int)__popcll(mask);
                if (wn >= (unsigned int)kWave) clip();
            }
        }
    }
    if (wn) clip();                                                 // the remainder, at the end of the wavefront's rows
    if constexpr (!EMIT) {
#pragma unroll
        for (int r = 0; r < kSpRows; r++)
            if (lane == r && row0 + r < n) offsets[row0 + r] = (int64_t)cnt[r];
    }
}

// ---------------------------------------------------------------- counts[n] -> offsets[n + 1], in place
constexpr int kSpItems = kSpTile / kSpThreads;

__global__ __launch_bounds__(kSpThreads) void k_sp_tile_sum(const int64_t *__restrict__ counts, int64_t n, unsigned long long *__restrict__ bsum)
{
    __shared__ unsigned long long sm[kSpWaves];
    const int64_t base = tile_item<kSpThreads, kSpItems>(blockIdx.x);
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < kSpItems; k++) {
        const int64_t i = base + (int64_t)k * kWave;
        if (i < n) s += (unsigned long long)counts[i];
    }
    s = tile_sum_u64<kSpThreads>(s, sm);
    if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

// every thread reads its items before it writes them: in place
__global__ __launch_bounds__(kSpThreads) void k_sp_offsets(int64_t *__restrict__ offsets, int64_t n, const unsigned long long *__restrict__ bsum_excl)
{
    __shared__ unsigned long long sm[kSpWaves];
    const int64_t base = tile_item<kSpThreads, kSpItems>(blockIdx.x);
    unsigned long long v[kSpItems], ex[kSpItems], total;
#pragma unroll
    for (int k = 0; k < kSpItems; k++) {
        const int64_t i = base + (int64_t)k * kWave;
        v[k] = i < n ? (unsigned long long)offsets[i] : 0ull;
    }
    tile_excl_scan_u64<kSpThreads, kSpItems>(v, ex, sm, &total);
    const unsigned long long before = bsum_excl[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kSpItems; k++) {
        const int64_t i = base + (int64_t)k * kWave;
        if (i < n) offsets[i] = (int64_t)(before + ex[k]);
    }
}

struct SparseWs {
    float4 *cb;                    // conservative bounding boxes of boxes2
    unsigned long long *bsum;      // hits per tile of kSpTile rows
};
SparseWs sparse_carve(WsCarver &w, int64_t n, int64_t m)
{
    SparseWs a;
    a.cb = w.take<float4>((size_t)m);
    a.bsum = w.take<unsigned long long>((size_t)d3d_divup(n, kSpTile));
    return a;
}

// the checks the two entries share, in the order of paired_check (boxpair.hip); *launch = there is something to do
int sparse_check(const void *b1, int64_t n, const void *b2, int64_t m, int32_t cols, int32_t iou_type, int32_t dtype, double threshold,
                 bool *launch)
{
    *launch = false;
    if (n < 0 || m < 0 || n > 0x7fffffffll || m > 0x7fffffffll || (cols != 5 && cols != 7)) return D3D_ERR_BAD_ARG;
    if (iou_type != D3D_IOU_BOX && iou_type != D3D_IOU_RBOX) return D3D_ERR_UNSUPPORTED;
    if (cols == 5 ? (dtype != D3D_F32 && dtype != D3D_F64 && dtype != D3D_F32_WIDE) : dtype != D3D_F32) return D3D_ERR_UNSUPPORTED;
    if (!(threshold >= 0) || !isfinite(threshold)) return D3D_ERR_BAD_ARG;
    if (n == 0 || m == 0) return D3D_OK;
    if (!b1 || !b2) return D3D_ERR_BAD_ARG;
    *launch = true;
    return D3D_OK;
}

// k_sp_aabb and k_sp_sweep<EMIT> for the call's element types, columns and method
template <bool EMIT>
int sparse_sweep(const void *b1, int64_t n, const void *b2, int64_t m, int32_t cols, int32_t iou_type, int32_t dtype, double threshold,
                 int64_t *offsets, int64_t *pairs, void *values, int64_t capacity, const SparseWs &a, hipStream_t st)
{
    auto run = [&](auto p, auto c) -> int {
        typedef typename decltype(p)::T T;
        typedef typename decltype(p)::B B;
        constexpr int COLS = decltype(c)::value;
        return dispatch(iou_type == D3D_IOU_RBOX, [&](auto rot) -> int {
            D3D_LAUNCH("k_sp_aabb", (k_sp_aabb<B, T, COLS, rot>), dim3((unsigned)d3d_divup(m, kSpThreads)), dim3(kSpThreads), 0, st,
                       (const B *)b2, m, a.cb);
            D3D_LAUNCH(EMIT ? "k_sp_sweep<emit>" : "k_sp_sweep<count>", (k_sp_sweep<B, T, COLS, rot, EMIT>),
                       dim3((unsigned)d3d_divup(n, kSpWaves * kSpRows)), dim3(kSpThreads), 0, st, (const B *)b1, n, (const B *)b2, m,
                       (const float4 *)a.cb, (B)threshold, offsets, pairs, (B *)values, capacity);
            return D3D_OK;
        });
    };
    if (cols == 7) return run(Prec<float>{}, std::integral_constant<int, 7>{});
    return dispatch_dtype<D3D_F32, D3D_F64, D3D_F32_WIDE>(dtype, [&](auto p) { return run(p, std::integral_constant<int, 5>{}); });
}

}  // namespace

extern "C" size_t d3d_iou_sparse_workspace_bytes(int64_t n, int64_t m)
{
    if (n < 0 || m < 0) return 0;
    WsCarver w(nullptr, 0);
    sparse_carve(w, n < 1 ? 1 : n, m < 1 ? 1 : m);
    return w.off;
}

extern "C" int d3d_iou_sparse_count(const void *boxes1, int64_t n, const void *boxes2, int64_t m, int32_t cols, int32_t iou_type,
                                    int32_t dtype, double threshold, int64_t *offsets, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    bool launch;
    if (const int rc = sparse_check(boxes1, n, boxes2, m, cols, iou_type, dtype, threshold, &launch); rc != D3D_OK) return rc;
    if (!launch) {                                                   // no pair: every offset is 0 (a fill, no kernel)
        if (offsets) D3D_HIP_CHECK(hipMemsetAsync(offsets, 0, (size_t)(n + 1) * sizeof(int64_t), st));
        return D3D_OK;
    }
    if (!offsets) return D3D_ERR_BAD_ARG;
    WsCarver w(workspace, workspace_bytes);
    const SparseWs a = sparse_carve(w, n, m);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    if (const int rc = sparse_sweep<false>(boxes1, n, boxes2, m, cols, iou_type, dtype, threshold, offsets, nullptr, nullptr, 0, a, st);
        rc != D3D_OK)
        return rc;
    const int64_t nb = d3d_divup(n, kSpTile);
    D3D_LAUNCH("k_sp_tile_sum", k_sp_tile_sum, dim3((unsigned)nb), dim3(kSpThreads), 0, st, (const int64_t *)offsets, n, a.bsum);
    D3D_LAUNCH("k_scan_tile_sums", k_scan_tile_sums<kSumsWhole>, dim3(1), dim3(1024), 0, st, a.bsum, nb, offsets + n);      // offsets[n] = K, 64 bits
    D3D_LAUNCH("k_sp_offsets", k_sp_offsets, dim3((unsigned)nb), dim3(kSpThreads), 0, st, offsets, n, (const unsigned long long *)a.bsum);
    return D3D_OK;
}

extern "C" int d3d_iou_sparse_emit(const void *boxes1, int64_t n, const void *boxes2, int64_t m, int32_t cols, int32_t iou_type,
                                   int32_t dtype, double threshold, const int64_t *offsets, int64_t capacity, int64_t *pairs,
                                   void *values, void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    bool launch;
    if (const int rc = sparse_check(boxes1, n, boxes2, m, cols, iou_type, dtype, threshold, &launch); rc != D3D_OK) return rc;
    if (capacity < 0) return D3D_ERR_BAD_ARG;
    if (!launch) return D3D_OK;
    if (!offsets) return D3D_ERR_BAD_ARG;
    WsCarver w(workspace, workspace_bytes);
    const SparseWs a = sparse_carve(w, n, m);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    // K is on the device: the entry reads the one word back (it waits for `stream`, i.e. for the count pass) before anything is written
    int64_t k = 0;
    D3D_HIP_CHECK(hipMemcpyAsync(&k, offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    D3D_HIP_CHECK(hipStreamSynchronize(st));
    if (capacity < k) return D3D_ERR_BAD_ARG;
    if (k == 0) return D3D_OK;
    if (!pairs || !values) return D3D_ERR_BAD_ARG;
    return sparse_sweep<true>(boxes1, n, boxes2, m, cols, iou_type, dtype, threshold, const_cast<int64_t *>(offsets), pairs, values, capacity, a, st);
}
