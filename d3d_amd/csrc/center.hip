// center.hip -- the centre head of CenterPoint / BEVFusion / OpenPCDet's CenterHead (the reference has no counterpart):
//   d3d_heatmap_peaks     the K best local maxima of a [B, C, H, W] heat map: CenterNet's max_pool2d + `==` + topk (OpenPCDet:
//                         two topk's) as an exact radix select; no pooled map, no keep mask, nothing read back
//   d3d_circle_nms        det3d's circle_nms (a numba loop on the host), per segment, one workgroup each
//   d3d_gaussian_heatmap  CenterNet's draw_gaussian over all boxes of a batch (OpenPCDet: a Python loop over boxes), one launch
// The rules are in include/d3d_hip.h; every output is integers, copies of input bits, or one rounded expression.
//
// The select.  Candidates (peaks above the threshold) are ranked by KeyBits<float>::desc of their value, ties by ascending flat
// index.  The k-th key is found exactly by three counting passes over the map -- the top 12 key bits, the next 12 inside the pivot
// bin, the last 8 -- each followed by one small workgroup per sample that walks the histogram (k_peak_pick).  Then the winners are
// compacted: every candidate above the pivot key, and of those equal to it the `need` lowest flat indices; the workgroups own
// runs of 1024 consecutive flat cells, so "lowest flat index" is a prefix sum over tiles: count -> scan -> emit, as camera.hip.
// One workgroup per sample finally orders the <= k winners on (key, flat index) with sort_lds and writes the four outputs.
// A constant map costs what any other map costs: five passes over the map.  Every pass recomputes the peak test from the map
// (it stays in L2 / Infinity Cache); the passes after the first test the cell's own key against the pivot first, and only the
// cells that can still matter look at their window.  The windows are read from global memory as they lie (consecutive lanes
// read consecutive cells of a row): a workgroup's run of flat cells crosses rows and planes, so it has no rectangular halo.
#include "lds_sort.hpp"

namespace {

// ---------------------------------------------------------------- heatmap_peaks
constexpr int kPeakMaxK = 4096;
constexpr int kPeakThreads = 256, kPeakItems = 4, kPeakTile = kPeakThreads * kPeakItems;
constexpr int kPeakBins = 4096;                 // levels 0 and 1: 12 bits; level 2: 8 bits (256 of the bins)
constexpr int kPeakSortThreads = 1024;
// per-sample select state (uint32 words)
enum { kStPrefix = 0, kStAbove = 1, kStTake = 2, kStNeed = 3, kStWords = 8 };

struct PeakDims {
    int32_t c, h, w;
    int32_t hw, chw;                            // h * w, c * h * w (<= 2^31 - 1)
    int32_t has_thr;
    float thr;
};

struct PeakWs {
    uint32_t *zeroed;                           // state[B][kStWords], hist[3][B][kPeakBins]: cleared by one memset
    size_t zeroed_bytes;
    uint32_t *state, *hist;
    unsigned long long *bsum;                   // [B][tiles]
    uint32_t *wkey, *widx;                      // [B][k] the winners, unordered
};

static PeakWs peak_carve(WsCarver &w, int64_t b, int64_t tiles, int64_t k)
{
    PeakWs a;
    const size_t words = (size_t)b * kStWords + (size_t)3 * b * kPeakBins;
    a.zeroed = w.take<uint32_t>(words);
    a.zeroed_bytes = words * sizeof(uint32_t);
    a.state = a.zeroed;
    a.hist = a.zeroed ? a.zeroed + (size_t)b * kStWords : nullptr;
    a.bsum = w.take<unsigned long long>((size_t)b * tiles);
    a.wkey = w.take<uint32_t>((size_t)b * k);
    a.widx = w.take<uint32_t>((size_t)b * k);
    return a;
}

template <class T> __device__ __forceinline__ float widen(T v) { return (float)v; }

// The value of flat cell `e` of a sample as fp32 and whether the cell is a candidate: v >= every value of its KS x KS window
// clipped to its plane (a NaN anywhere in the window, v itself included, fails a comparison) and v > thr where there is one.
// SKIP(key): the caller has no use for a candidate with that key; the window is then not read.
template <class T, int KS, class Skip>
__device__ __forceinline__ bool peak_candidate(const T *__restrict__ sample, const PeakDims &d, int32_t e, uint32_t &key, Skip skip)
{
    const float v = widen(sample[e]);
    key = KeyBits<float>::desc(v);
    if (!(v == v) || (d.has_thr && !(v > d.thr)) || skip(key)) return false;
    if (KS == 1) return true;
    constexpr int R = KS / 2;
    const int32_t plane = e / d.hw, rem = e - plane * d.hw, y = rem / d.w, x = rem - y * d.w;
    const T *p = sample + (e - rem);
    bool ok = true;
#pragma unroll
    for (int dy = -R; dy <= R; dy++) {
        const int32_t yy = y + dy;
        if (yy < 0 || yy >= d.h) continue;
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            const int32_t xx = x + dx;
            if ((dy == 0 && dx == 0) || xx < 0 || xx >= d.w) continue;
            ok = ok && (v >= widen(p[yy * d.w + xx]));
        }
    }
    return ok;
}

// level 0: bin = key >> 20; level 1: keys with the pivot's top 12 bits, bin = (key >> 8) & 4095; level 2: keys with its top 24
// bits, bin = key & 255.  hist[(level * B + b) * kPeakBins + bin] += the candidates of the tile.
template <class T, int KS>
__global__ __launch_bounds__(kPeakThreads) void k_peak_hist(const T *__restrict__ heat, PeakDims d, int level,
                                                            const uint32_t *__restrict__ state, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t sh[kPeakBins];
    const int b = blockIdx.y;
    const int bins = level == 2 ? 256 : kPeakBins;
    const uint32_t keep_mask = level == 0 ? 0u : level == 1 ? 0xfff00000u : 0xffffff00u;      // the key bits that must equal the pivot's
    const int bin_shift = level == 0 ? 20 : level == 1 ? 8 : 0;
    const uint32_t prefix = state[(int64_t)b * kStWords + kStPrefix];
    if (level > 0 && state[(int64_t)b * kStWords + kStTake] == 0) return;   // no candidates at all (workgroup-uniform)
    for (int i = threadIdx.x; i < bins; i += kPeakThreads) sh[i] = 0;
    __syncthreads();
    const T *sample = heat + (int64_t)b * d.chw;
    const int64_t base = tile_item<kPeakThreads, kPeakItems>(blockIdx.x);
#pragma unroll
    for (int j = 0; j < kPeakItems; j++) {
        const int64_t e = base + (int64_t)j * kWave;
        if (e >= d.chw) continue;
        uint32_t key;
        const bool cand = peak_candidate<T, KS>(sample, d, (int32_t)e, key, [&](uint32_t q) { return ((q ^ prefix) & keep_mask) != 0; });
        if (cand) atomicAdd(&sh[(key >> bin_shift) & (uint32_t)(bins - 1)], 1u);
    }
    __syncthreads();
    uint32_t *out = hist + ((int64_t)level * gridDim.y + b) * kPeakBins;
    for (int i = threadIdx.x; i < bins; i += kPeakThreads) {
        const uint32_t v = sh[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// workgroup b walks sample b's histogram of `level`.  With take = min(k, candidates) (fixed at level 0) it finds the bin that
// holds the take-th smallest key, appends the bin to the pivot's prefix and adds the candidates of the bins below it to `above`;
// after level 2 the prefix is the pivot key itself, `above` the candidates strictly better and need = take - above those taken
// from the ties of the pivot key.  No candidates: take = need = 0 and the pivot stays 0, the key no candidate has (NaN's).
__global__ __launch_bounds__(1024) void k_peak_pick(uint32_t *__restrict__ state, const uint32_t *__restrict__ hist, int level, int k,
                                                     int32_t *__restrict__ counts)
{
    __shared__ unsigned long long smem[1024 / kWave];
    const int b = blockIdx.x;
    uint32_t *st = state + (int64_t)b * kStWords;
    const uint32_t *h = hist + ((int64_t)level * gridDim.x + b) * kPeakBins;
    const int bin_shift = level == 0 ? 20 : level == 1 ? 8 : 0;
    uint32_t v[4];
    unsigned long long mine = 0, total;
#pragma unroll
    for (int j = 0; j < 4; j++) { v[j] = h[threadIdx.x * 4 + j]; mine += v[j]; }
    unsigned long long below = block_excl_scan_u64<1024>(mine, &total, smem);
    uint32_t take = st[kStTake];
    const uint32_t above = st[kStAbove], prefix = st[kStPrefix];
    __syncthreads();                                                   // (everyone has read the state the winner rewrites)
    if (level == 0) {
        take = total < (unsigned long long)k ? (uint32_t)total : (uint32_t)k;
        if (threadIdx.x == 0) {
            st[kStTake] = take;
            counts[b] = (int32_t)take;
        }
    }
    if (take == 0) return;
    below += above;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (below < take && take <= below + v[j]) {                    // (exactly one bin of the level)
            st[kStPrefix] = prefix | ((uint32_t)(threadIdx.x * 4 + j) << bin_shift);
            st[kStAbove] = (uint32_t)below;
            if (level == 2) st[kStNeed] = take - (uint32_t)below;
        }
        below += v[j];
    }
}

// (candidates above the pivot : 32 | candidates equal to it : 32) of a cell
template <class T, int KS>
__device__ __forceinline__ unsigned long long peak_flags(const T *__restrict__ sample, const PeakDims &d, int64_t e, uint32_t pivot,
                                                         uint32_t &key)
{
    key = 0;
    if (e >= d.chw) return 0ull;
    if (!peak_candidate<T, KS>(sample, d, (int32_t)e, key, [&](uint32_t q) { return q > pivot; })) return 0ull;
    return key < pivot ? 1ull << 32 : 1ull;
}

template <class T, int KS>
__global__ __launch_bounds__(kPeakThreads) void k_peak_count(const T *__restrict__ heat, PeakDims d, const uint32_t *__restrict__ state,
                                                             unsigned long long *__restrict__ bsum)
{
    __shared__ unsigned long long sm[kPeakThreads / kWave];
    const int b = blockIdx.y;
    const uint32_t pivot = state[(int64_t)b * kStWords + kStPrefix];
    const T *sample = heat + (int64_t)b * d.chw;
    const int64_t base = tile_item<kPeakThreads, kPeakItems>(blockIdx.x);
    unsigned long long s = 0;
#pragma unroll
    for (int j = 0; j < kPeakItems; j++) {
        uint32_t key;
        s += peak_flags<T, KS>(sample, d, base + (int64_t)j * kWave, pivot, key);
    }
    s = tile_sum_u64<kPeakThreads>(s, sm);
    if (threadIdx.x == 0) bsum[(int64_t)b * gridDim.x + blockIdx.x] = s;
}

// the same flags again (the same expressions on the same map), a scan inside the workgroup, and the winners' stores: a candidate
// above the pivot goes to the slot of its rank among those (below `above`), a tie of the pivot key to above + its rank among the
// ties when that rank is below `need`
template <class T, int KS>
__global__ __launch_bounds__(kPeakThreads) void k_peak_emit(const T *__restrict__ heat, PeakDims d, const uint32_t *__restrict__ state,
                                                            const unsigned long long *__restrict__ bsum_excl, int k,
                                                            uint32_t *__restrict__ wkey, uint32_t *__restrict__ widx)
{
    __shared__ unsigned long long sm[kPeakThreads / kWave];
    const int b = blockIdx.y;
    const uint32_t *st = state + (int64_t)b * kStWords;
    const uint32_t pivot = st[kStPrefix], above = st[kStAbove], need = st[kStNeed];
    const T *sample = heat + (int64_t)b * d.chw;
    const int64_t base = tile_item<kPeakThreads, kPeakItems>(blockIdx.x);
    unsigned long long f[kPeakItems], ex[kPeakItems], total;
    uint32_t key[kPeakItems];
#pragma unroll
    for (int j = 0; j < kPeakItems; j++) f[j] = peak_flags<T, KS>(sample, d, base + (int64_t)j * kWave, pivot, key[j]);
    tile_excl_scan_u64<kPeakThreads, kPeakItems>(f, ex, sm, &total);
    const unsigned long long before = bsum_excl[(int64_t)b * gridDim.x + blockIdx.x];
#pragma unroll
    for (int j = 0; j < kPeakItems; j++) {
        if (!f[j]) continue;
        const unsigned long long off = before + ex[j];
        const uint32_t lt = (uint32_t)(off >> 32), eq = (uint32_t)off;
        uint32_t slot;
        if (f[j] >> 32) slot = lt;
        else if (eq < need) slot = above + eq;
        else continue;
        if (slot >= (uint32_t)k) continue;                            // (cannot happen: above + need = take <= k)
        wkey[(int64_t)b * k + slot] = key[j];
        widx[(int64_t)b * k + slot] = (uint32_t)(base + (int64_t)j * kWave);
    }
}

// workgroup b orders sample b's winners on (key, flat index) and writes the outputs.  BITS: the element of the map as an
// unsigned integer -- the scores are copies of the map's own bits.  min(npad, 1024) threads (sort_lds reads an entry per thread and
// slot); LDS: 16 bytes per padded entry (64 KB at 4096).
template <class BITS, int EPT>
__global__ __launch_bounds__(kPeakSortThreads) void k_peak_sort(const BITS *__restrict__ heat, PeakDims d, int k, int npad,
                                                                const uint32_t *__restrict__ state, const uint32_t *__restrict__ wkey,
                                                                const uint32_t *__restrict__ widx, BITS neg_inf, BITS *__restrict__ scores,
                                                                int32_t *__restrict__ classes, int32_t *__restrict__ ys,
                                                                int32_t *__restrict__ xs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char peak_lds[];
    const int b = blockIdx.x;
    const int take = (int)state[(int64_t)b * kStWords + kStTake];
    uint32_t *d0 = reinterpret_cast<uint32_t *>(peak_lds), *d1 = d0 + npad, *i0 = d1 + npad, *i1 = i0 + npad, *rd, *ri;
    for (int e = threadIdx.x; e < npad; e += (int)blockDim.x) {
        const bool real = e < take;
        d0[e] = real ? wkey[(int64_t)b * k + e] : kPadKey<uint32_t>;  // padding: last, unique (a flat index is below 2^31)
        i0[e] = real ? widx[(int64_t)b * k + e] : kPadIndex + (uint32_t)e;
    }
    __syncthreads();
    sort_lds<EPT>(d0, i0, d1, i1, npad, &rd, &ri);
    const BITS *sample = heat + (int64_t)b * d.chw;
    for (int r = threadIdx.x; r < k; r += (int)blockDim.x) {
        const int64_t o = (int64_t)b * k + r;
        if (r < take) {
            const int32_t e = (int32_t)ri[r], plane = e / d.hw, rem = e - plane * d.hw, y = rem / d.w;
            scores[o] = sample[e];
            classes[o] = plane;
            ys[o] = y;
            xs[o] = rem - y * d.w;
        } else {
            scores[o] = neg_inf;
            classes[o] = ys[o] = xs[o] = -1;
        }
    }
}

// ---------------------------------------------------------------- circle_nms
constexpr int kCircleMax = 4096;
constexpr int kCircleThreads = 1024;

// det3d's test, every operation one rounding in T (the build does not contract); a NaN d2 is no hit
template <class T> __device__ __forceinline__ bool circle_hit(T xi, T yi, T xj, T yj, T t)
{
    const T dx = xi - xj, dy = yi - yj;
    const T d2 = dx * dx + dy * dy;
    return d2 <= t;
}

template <class T> static __host__ __device__ inline size_t circle_lds_bytes(int npad)
{
    const size_t sort = (size_t)npad * 2 * (sizeof(typename KeyBits<T>::U) + sizeof(uint32_t));
    const size_t xy = (size_t)npad * 2 * sizeof(T);
    return (sort > xy ? sort : xy) + (size_t)(kCircleMax / kWave) * sizeof(unsigned long long);
}

// One workgroup per segment, rows perm[seg0 .. seg1) (perm NULL: the rows themselves).  Rank p of the segment's score order
// belongs to wavefront (p / 64) % NW, lane p % 64, slot p / (64 NW), NW = min(npad, 1024) / 64 wavefronts: the state of a block of
// 64 ranks lives in the registers of ONE wavefront.  Block c: its wavefront resolves it alone -- row r, unless suppressed by then, suppresses the later lanes within t of
// it: one ballot per open row -- and publishes the kept word; after the barrier every wavefront applies the block's kept rows to
// the later blocks it owns.  One barrier per block; a suppressed row never suppresses, so a resolved block is final.
template <class T, int EPT>
__global__ __launch_bounds__(kCircleThreads) void k_circle_nms(const T *__restrict__ centers, int stride, const T *__restrict__ scores,
                                                               const int64_t *__restrict__ perm, const int64_t *__restrict__ seg_offsets,
                                                               T thr, int max_keep, int npad, uint8_t *__restrict__ keep)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char circle_lds[];
    typedef typename KeyBits<T>::U U;
    const int64_t seg0 = seg_offsets[blockIdx.x], len = seg_offsets[blockIdx.x + 1] - seg0;
    if (len <= 0 || len > npad || npad > EPT * (int)blockDim.x) return;   // (above the cap: refused by the entry, nothing is touched)
    const int n = (int)len, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const size_t body = circle_lds_bytes<T>(npad) - (size_t)(kCircleMax / kWave) * sizeof(unsigned long long);
    unsigned long long *keptw = reinterpret_cast<unsigned long long *>(circle_lds + body);
    // ---- the order: KeyBits composites with the LOCAL index (ties: ascending position, i.e. ascending row for a stable perm)
    U *d0 = reinterpret_cast<U *>(circle_lds), *d1 = d0 + npad, *rd;
    uint32_t *i0 = reinterpret_cast<uint32_t *>(d1 + npad), *i1 = i0 + npad, *ri;
    fill_desc_keys(d0, i0, npad, n, [&](int e) { return scores[perm ? perm[seg0 + e] : seg0 + e]; });
    sort_lds<EPT>(d0, i0, d1, i1, npad, &rd, &ri);
    // ---- the rows of this thread's ranks; the coordinates by rank go where the sort was
    const int nchunks = (n + kWave - 1) / kWave;
    int64_t row[EPT];
    T x[EPT], y[EPT];
    bool sup[EPT];
#pragma unroll
    for (int u = 0; u < EPT; u++) {
        const int p = (wave + u * nw) * kWave + lane;
        sup[u] = p >= n;                                               // (ranks past n: suppressed, NaN coordinates, never a hit)
        row[u] = 0;
        x[u] = y[u] = (T)NAN;
        if (p < n) {
            const uint32_t local = ri[p];
            row[u] = perm ? perm[seg0 + local] : seg0 + local;
            x[u] = centers[row[u] * stride];
            y[u] = centers[row[u] * stride + 1];
        }
    }
    __syncthreads();
    T *xs = reinterpret_cast<T *>(circle_lds), *ys = xs + npad;
#pragma unroll
    for (int u = 0; u < EPT; u++) {
        const int p = (wave + u * nw) * kWave + lane;
        if (p < npad) { xs[p] = x[u]; ys[p] = y[u]; }
    }
    // ---- the sweep
    for (int c = 0; c < nchunks; c++) {
        if (wave == c % nw) {
#pragma unroll
            for (int u = 0; u < EPT; u++) {
                if (u != c / nw) continue;
                unsigned long long s = __ballot(sup[u]);
#pragma unroll 4
                for (int r = 0; r < kWave - 1; r++) {
                    if ((s >> r) & 1ull) continue;                     // (wave-uniform: a suppressed row suppresses nothing)
                    const T xr = wave_readlane(x[u], r), yr = wave_readlane(y[u], r);
                    s |= __ballot(lane > r && circle_hit(xr, yr, x[u], y[u], thr));
                }
                sup[u] = (s >> lane) & 1ull;
                if (lane == 0) keptw[c] = ~s;
            }
        }
        __syncthreads();                                               // keptw[c] and, the first time, xs / ys are written
        const unsigned long long kept = keptw[c];
        for (unsigned long long m = kept; m; m &= m - 1) {
            const int q = c * kWave + __builtin_ctzll(m);
            const T xq = xs[q], yq = ys[q];
#pragma unroll
            for (int u = 0; u < EPT; u++)
                if (wave + u * nw > c && !sup[u] && circle_hit(xq, yq, x[u], y[u], thr)) sup[u] = true;
        }
    }
    // ---- max_keep: a kept rank stays when fewer than max_keep kept ranks precede it (every keptw word is final)
#pragma unroll
    for (int u = 0; u < EPT; u++) {
        const int chunk = wave + u * nw, p = chunk * kWave + lane;
        if (p >= n) continue;
        bool stay = !sup[u];
        if (stay && max_keep < n) {
            int before = __popcll(keptw[chunk] & ((1ull << lane) - 1ull));
            for (int cc = 0; cc < chunk; cc++) before += __popcll(keptw[cc]);
            stay = before < max_keep;
        }
        keep[row[u]] = stay ? 1 : 0;
    }
}

// ---------------------------------------------------------------- gaussian_heatmap
constexpr int kDrawThreads = 256, kDrawTileW = 64, kDrawTileH = 16, kDrawRows = kDrawTileH * kDrawTileW / kDrawThreads;

// A workgroup owns a 16 x 64 tile of one class plane of one sample.  The sample's boxes pass through LDS 256 at a time; a
// wavefront keeps, by ballot, the boxes of the plane's class whose window meets the tile.  Every cell of the tile is stored once.
__global__ __launch_bounds__(kDrawThreads) void k_gaussian_heatmap(const int32_t *__restrict__ centers, const int32_t *__restrict__ radii,
                                                                   const int32_t *__restrict__ classes,
                                                                   const int64_t *__restrict__ offsets, int64_t m, int c_total, int h,
                                                                   int w, int tiles_x, float *__restrict__ out)
{
    __shared__ int4 sbox[kDrawThreads / kWave][kWave];
    __shared__ int scnt[kDrawThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int b = blockIdx.z, cls = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * kDrawTileW, y0 = ty * kDrawTileH;
    const int x1 = min(x0 + kDrawTileW, w) - 1, y1 = min(y0 + kDrawTileH, h) - 1;      // the tile's last column and row
    const int64_t m0 = offsets ? offsets[b] : 0, m1 = offsets ? offsets[b + 1] : m;
    const int px = x0 + lane;
    float best[kDrawRows];
#pragma unroll
    for (int j = 0; j < kDrawRows; j++) best[j] = 0.f;
    for (int64_t i0 = m0; i0 < m1; i0 += kDrawThreads) {
        const int64_t i = i0 + threadIdx.x;
        int4 box = make_int4(0, 0, 0, 0);
        bool hit = false;
        if (i < m1) {
            box = make_int4(centers[2 * i], centers[2 * i + 1], radii[i], 0);
            // (int64: a centre may lie anywhere in int32; r is in 0 .. 4095 by the entry's contract with its caller)
            hit = classes[i] == cls && (int64_t)box.x + box.z >= x0 && (int64_t)box.x - box.z <= x1 &&
                  (int64_t)box.y + box.z >= y0 && (int64_t)box.y - box.z <= y1;
        }
        const unsigned long long mask = __ballot(hit);
        if (hit) sbox[wave][__popcll(mask & ((1ull << lane) - 1ull))] = box;
        if (lane == 0) scnt[wave] = __popcll(mask);
        __syncthreads();
        for (int wv = 0; wv < kDrawThreads / kWave; wv++) {
            const int cnt = scnt[wv];
            for (int q = 0; q < cnt; q++) {
                const int4 g = sbox[wv][q];
                const int64_t dx64 = (int64_t)px - g.x;                // (a centre may lie anywhere: |dx| <= r before dx is narrowed)
                if (px > x1 || dx64 > g.z || dx64 < -g.z) continue;
                const int dx = (int)dx64;
                const int side = 2 * g.z + 1;
                const double den = (double)(side * side);
#pragma unroll
                for (int j = 0; j < kDrawRows; j++) {
                    const int64_t dy64 = (int64_t)(y0 + wave + j * (kDrawThreads / kWave)) - g.y;
                    if (dy64 > g.z || dy64 < -g.z) continue;
                    const int dy = (int)dy64, d2 = dx * dx + dy * dy;
                    best[j] = fmaxf(best[j], (float)exp(-(double)(18 * d2) / den));
                }
            }
        }
        __syncthreads();
    }
    if (px > x1) return;
    float *plane = out + ((int64_t)b * c_total + cls) * h * (int64_t)w;
#pragma unroll
    for (int j = 0; j < kDrawRows; j++) {
        const int py = y0 + wave + j * (kDrawThreads / kWave);
        if (py <= y1) plane[(int64_t)py * w + px] = best[j];
    }
}

}  // namespace

// ---------------------------------------------------------------- entries
extern "C" int32_t d3d_heatmap_peaks_max(void) { return kPeakMaxK; }

static bool peak_shape_ok(int64_t b, int64_t c, int64_t h, int64_t w, int64_t k)
{
    if (b < 0 || c < 1 || h < 1 || w < 1 || k < 1) return false;
    if (c > 0x7fffffffll || h > 0x7fffffffll || w > 0x7fffffffll) return false;
    return true;
}
static bool peak_shape_supported(int64_t b, int64_t c, int64_t h, int64_t w, int64_t k)
{
    if (k > kPeakMaxK || b > 65535) return false;
    if (c * h > 0x7fffffffll || c * h * w > 0x7fffffffll) return false;       // (c, h, w <= 2^31 - 1: the products fit int64)
    return true;
}

extern "C" size_t d3d_heatmap_peaks_workspace_bytes(int64_t b, int64_t c, int64_t h, int64_t w, int32_t k)
{
    if (!peak_shape_ok(b, c, h, w, k) || !peak_shape_supported(b, c, h, w, k)) return 0;
    WsCarver carver(nullptr, 0);
    peak_carve(carver, b, d3d_divup(c * h * w, kPeakTile), k);
    return carver.off + 256;
}

// CenterNet's _nms + _topk (max_pool2d, ==, topk; OpenPCDet's centernet_utils._topk: two topk's) on a [b, c, h, w] map.
extern "C" int d3d_heatmap_peaks(const void *heat, int64_t b, int64_t c, int64_t h, int64_t w, int32_t dtype, int32_t k, int32_t kernel,
                                 int32_t has_threshold, float threshold, void *scores, int32_t *classes, int32_t *ys, int32_t *xs,
                                 int32_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!peak_shape_ok(b, c, h, w, k) || (has_threshold != 0 && has_threshold != 1)) return D3D_ERR_BAD_ARG;
    if (kernel != 1 && kernel != 3 && kernel != 5 && kernel != 7) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F16 && dtype != D3D_BF16) return D3D_ERR_UNSUPPORTED;
    if (!peak_shape_supported(b, c, h, w, k)) return D3D_ERR_UNSUPPORTED;
    if (b == 0) return D3D_OK;
    if (!heat || !scores || !classes || !ys || !xs || !counts) return D3D_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < d3d_heatmap_peaks_workspace_bytes(b, c, h, w, k)) return D3D_ERR_WORKSPACE;
    const int64_t tiles = d3d_divup(c * h * w, kPeakTile);
    WsCarver carver(workspace, workspace_bytes);
    const PeakWs a = peak_carve(carver, b, tiles, k);
    if (!carver.ok()) return D3D_ERR_WORKSPACE;
    PeakDims d;
    d.c = (int32_t)c; d.h = (int32_t)h; d.w = (int32_t)w; d.hw = (int32_t)(h * w); d.chw = (int32_t)(c * h * w);
    d.has_thr = has_threshold; d.thr = threshold;
    const dim3 grid((unsigned)tiles, (unsigned)b);
    D3D_HIP_CHECK(hipMemsetAsync(a.zeroed, 0, a.zeroed_bytes, st));
    const int rc = dispatch_dtype<D3D_F32, D3D_F16, D3D_BF16>(dtype, [&](auto p) -> int {
        typedef typename decltype(p)::T T;
        return dispatch_int<1, 3, 5, 7>(kernel, [&](auto ks) -> int {
            constexpr int KS = decltype(ks)::value;
            for (int level = 0; level < 3; level++) {
                D3D_LAUNCH("k_peak_hist", (k_peak_hist<T, KS>), grid, dim3(kPeakThreads), 0, st, (const T *)heat, d, level, a.state, a.hist);
                D3D_LAUNCH("k_peak_pick", k_peak_pick, dim3((unsigned)b), dim3(1024), 0, st, a.state, a.hist, level, (int)k, counts);
            }
            D3D_LAUNCH("k_peak_count", (k_peak_count<T, KS>), grid, dim3(kPeakThreads), 0, st, (const T *)heat, d, a.state, a.bsum);
            D3D_LAUNCH("k_scan_tile_sums", k_scan_tile_sums<kSumsNone>, dim3((unsigned)b), dim3(1024), 0, st, a.bsum, tiles, (int64_t *)nullptr);
            D3D_LAUNCH("k_peak_emit", (k_peak_emit<T, KS>), grid, dim3(kPeakThreads), 0, st, (const T *)heat, d, a.state, a.bsum, (int)k, a.wkey,
                       a.widx);
            return D3D_OK;
        });
    });
    if (rc != D3D_OK) return rc;
    const int npad = sort_lds_pad(k);
    const size_t lds = (size_t)npad * 16;
    return dispatch(dtype == D3D_F32, [&](auto wide) -> int {
        typedef typename std::conditional<decltype(wide)::value, uint32_t, uint16_t>::type BITS;
        const BITS neg_inf = (BITS)(dtype == D3D_F32 ? 0xff800000u : dtype == D3D_F16 ? 0xfc00u : 0xff80u);
        return dispatch(npad > kPeakSortThreads, [&](auto big) -> int {
            constexpr int EPT = decltype(big)::value ? 4 : 1;
            D3D_LAUNCH("k_peak_sort", (k_peak_sort<BITS, EPT>), dim3((unsigned)b), dim3((unsigned)(npad < kPeakSortThreads ? npad : kPeakSortThreads)), lds, st, (const BITS *)heat, d, (int)k,
                       npad, a.state, a.wkey, a.widx, neg_inf, (BITS *)scores, classes, ys, xs);
            return D3D_OK;
        });
    });
}

extern "C" int32_t d3d_circle_nms_max(void) { return kCircleMax; }

// det3d's circle_nms (det3d/core/utils/circle_nms_jit.py, a numba loop on the host; OpenPCDet copies to the host for it), inside
// every segment of a batch.
extern "C" int d3d_circle_nms(const void *centers, int32_t stride, const void *scores, const int64_t *perm, const int64_t *seg_offsets,
                              int64_t n, int64_t segments, int32_t max_segment, int32_t dtype, double dist2_threshold, int32_t max_keep,
                              uint8_t *keep, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || segments < 0 || stride < 2 || max_segment < 0 || max_keep < 0) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64) return D3D_ERR_UNSUPPORTED;
    if (max_segment > kCircleMax || segments > 0x7fffffffll || n > 0x7fffffffll) return D3D_ERR_UNSUPPORTED;
    if (n == 0 || segments == 0 || max_segment == 0) return D3D_OK;
    if (!centers || !scores || !seg_offsets || !keep) return D3D_ERR_BAD_ARG;
    const int npad = sort_lds_pad(max_segment);
    return dispatch_dtype<D3D_F32, D3D_F64>(dtype, [&](auto p) -> int {
        typedef typename decltype(p)::T T;
        return dispatch(npad > kCircleThreads, [&](auto big) -> int {
            constexpr int EPT = decltype(big)::value ? 4 : 1;
            const size_t lds = circle_lds_bytes<T>(npad);
            if (lds > 65536)
                D3D_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_circle_nms<T, EPT>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            D3D_LAUNCH("k_circle_nms", (k_circle_nms<T, EPT>), dim3((unsigned)segments), dim3((unsigned)(npad < kCircleThreads ? npad : kCircleThreads)), lds, st, (const T *)centers,
                       (int)stride, (const T *)scores, perm, seg_offsets, (T)dist2_threshold, (int)max_keep, npad, keep);
            return D3D_OK;
        });
    });
}

// CenterNet's draw_umich_gaussian over every box of a batch (OpenPCDet's centernet_utils.draw_gaussian_to_heatmap, called per box
// from a Python loop in CenterHead.assign_target_of_single_head).
extern "C" int d3d_gaussian_heatmap(const int32_t *centers, const int32_t *radii, const int32_t *classes, const int64_t *offsets, int64_t m,
                                    int64_t b, int64_t c, int64_t h, int64_t w, float *out, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (m < 0 || b < 0 || c < 0 || h < 0 || w < 0) return D3D_ERR_BAD_ARG;
    if (!offsets && b > 1) return D3D_ERR_BAD_ARG;                        // (no offsets: one sample holds every box)
    if (b > 65535 || c > 65535 || h > (1 << 30) || w > (1 << 30) || m > 0x7fffffffll) return D3D_ERR_UNSUPPORTED;
    const int64_t tiles_x = d3d_divup(w, kDrawTileW), tiles_y = d3d_divup(h, kDrawTileH);
    if (tiles_x * tiles_y > 0x7fffffffll) return D3D_ERR_UNSUPPORTED;
    if (b == 0 || c == 0 || h == 0 || w == 0) return D3D_OK;
    if (!out || (m > 0 && (!centers || !radii || !classes))) return D3D_ERR_BAD_ARG;
    D3D_LAUNCH("k_gaussian_heatmap", k_gaussian_heatmap, dim3((unsigned)(tiles_x * tiles_y), (unsigned)c, (unsigned)b), dim3(kDrawThreads), 0,
               st, centers, radii, classes, offsets, m, (int)c, (int)h, (int)w, (int)tiles_x, out);
    return D3D_OK;
}
