// segeval.hip -- SegmentationEvaluator.calc_stats of the reference (d3d/benchmarks.pyx:977-1075: collect_labels and
// collect_labels_pano) for F stacked frames in one call.
//
// The reference walks every point and updates C++ unordered_maps; here the same counts are a histogram of 64-bit pair keys
//   frame(16) << 48 | gt_key(24) << 24 | pred_key(24),   gt_key = label << 16 | id  (label in classes)
//                                                                = background << 16 (otherwise; the id is dropped, :1000-1007)
// and everything else -- the semantic counts, the two marginals, the matching -- is derived from that histogram.
//
//   k_seg_init    zero the seven [F, 256] outputs, the fixed-point IoU sums and (panoptic) the three global tables
//   k_seg_points  one pass over the points (16 per lane, 16-byte loads where the pointers allow): run-length merge in registers,
//                 then an LDS open-addressing table per workgroup.  Its flush adds the semantic counts (integer atomics) and,
//                 panoptic, inserts into the global pair table and the gt / pred marginal tables (64-bit CAS).  A point whose
//                 LDS probe sequence is full goes straight to the global tables: no status, no retry.
//   k_seg_match   (panoptic) one lane per distinct pair: the filters and the IoU test of :1032-1063
//   k_seg_final   (panoptic) one lane per distinct gt / pred key: ifn / ifp (:1064-1075); the IoU sums to fp32
//
// Semantic counts from the pair keys: with g' / p' the labels of the keys (the label if in classes, else background), for
// g, p != background  g == p <=> g' == p', so tp / fn / fp of :977-987 are sums of pair counts.
//
// cumiou without float atomics and independent of order: a matched IoU is an fp32 value in (0.5, 1], an integer multiple of
// 2^-24, so iou * 2^24 is an exact integer and the per-(frame, class) sums are exact u64 atomics.  The stored fp32 is that
// exact sum rounded once; two runs give the same bits.  (The reference adds fp32 values in hash-map order: its last bits
// depend on that order.)
//
// The reference's "background subtraction" (:1055-1056) only runs when find() has just failed, so it subtracts the 0 that
// operator[] inserts: total = g + p - inter always, which is what k_seg_match computes.
#include "common.hpp"

namespace {
typedef unsigned long long u64;

constexpr int kSegThreads = 256;
constexpr int kSegPerLane = 16;                              // points per lane and step (one 16-byte load of labels)
constexpr int kSegStep = kSegThreads * kSegPerLane;          // points per workgroup and step
constexpr int kSegLdsSlots = 2048;                           // LDS table: 16 KiB keys + 8 KiB counts
constexpr int kSegLdsProbes = 32;
constexpr int kSegMaxBlocks = 1024;
constexpr u64 kSegEmpty = ~0ull;                             // never a key: frame < 0xffff
constexpr uint32_t kSegMatched = 0x80000000u;                // flag bit in a marginal count (counts < 2^31)

struct SegTables {
    u64 *pair_key, *gt_key, *pred_key;
    uint32_t *pair_cnt, *gt_cnt, *pred_cnt;
    u64 cap;                                                 // slots per table
    u64 *cumfix;                                             // [F, 256] sums of iou * 2^24
};
struct SegOut {
    int32_t *tp, *fp, *fn, *itp, *ifp, *ifn;
    float *cumiou;
};
struct SegArgs {
    uint32_t mask[8];                                        // class membership, 256 bits
    int32_t background, min_points, pano;
};

__device__ __forceinline__ u64 seg_mix(u64 h)
{
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

// add `c` to key's count in a global table (keys never change once set: a stale read is corrected by the CAS)
__device__ __forceinline__ void seg_global_add(u64 *keys, uint32_t *cnts, u64 cap, u64 key, uint32_t c)
{
    u64 s = __umul64hi(seg_mix(key), cap);
    for (u64 q = 0; q < cap; q++) {                          // (the table holds at most n < cap keys: it never fills)
        u64 k = keys[s];
        if (k == kSegEmpty) {
            k = atomicCAS(&keys[s], kSegEmpty, key);
            if (k == kSegEmpty) k = key;
        }
        if (k == key) { atomicAdd(&cnts[s], c); return; }
        s = s + 1 == cap ? 0 : s + 1;
    }
}

// slot of a key that is in the table (after the kernel that inserted it); cap if it is not
__device__ __forceinline__ u64 seg_global_find(const u64 *keys, u64 cap, u64 key)
{
    u64 s = __umul64hi(seg_mix(key), cap);
    for (u64 q = 0; q < cap; q++) {
        if (keys[s] == key) return s;
        s = s + 1 == cap ? 0 : s + 1;
    }
    return cap;
}

// one (pair key, count) of a workgroup -- or of a single point run when its LDS probes found no slot
__device__ __forceinline__ void seg_record(const SegTables &t, const SegOut &o, const SegArgs &a, u64 key, uint32_t c)
{
    const uint32_t f = (uint32_t)(key >> 48), gl = (uint32_t)(key >> 40) & 0xff, pl = (uint32_t)(key >> 16) & 0xff;
    const size_t base = (size_t)f * 256;
    const uint32_t bg = (uint32_t)a.background;
    if (gl != bg) atomicAdd(gl == pl ? &o.tp[base + gl] : &o.fn[base + gl], (int32_t)c);           // :979-983
    if (pl != bg && pl != gl) atomicAdd(&o.fp[base + pl], (int32_t)c);                              // :984-985
    if (a.pano) {                                                                                  // :1012-1027
        seg_global_add(t.pair_key, t.pair_cnt, t.cap, key, c);
        seg_global_add(t.gt_key, t.gt_cnt, t.cap, (u64)f << 24 | ((key >> 24) & 0xffffff), c);
        seg_global_add(t.pred_key, t.pred_cnt, t.cap, (u64)f << 24 | (key & 0xffffff), c);
    }
}

__device__ __forceinline__ void seg_lds_add(u64 *skey, uint32_t *scnt, const SegTables &t, const SegOut &o, const SegArgs &a,
                                            u64 key, uint32_t c)
{
    const uint32_t h = (uint32_t)seg_mix(key);
    for (int q = 0; q < kSegLdsProbes; q++) {
        const uint32_t s = (h + q) & (kSegLdsSlots - 1);
        u64 k = skey[s];
        if (k == kSegEmpty) {
            k = atomicCAS(&skey[s], kSegEmpty, key);
            if (k == kSegEmpty) k = key;
        }
        if (k == key) { atomicAdd(&scnt[s], c); return; }
    }
    seg_record(t, o, a, key, c);
}

// largest f in [lo, hi] with off[f] <= i (lo if none): the frame of point i, empty frames skipped
__device__ __forceinline__ int seg_frame_of(const int64_t *off, int64_t i, int lo, int hi)
{
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_seg_init(SegTables t, SegOut o, int64_t fcells, int pano)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)fcells; i += stride) {
        o.tp[i] = 0; o.fp[i] = 0; o.fn[i] = 0;
        o.itp[i] = 0; o.ifp[i] = 0; o.ifn[i] = 0;
        o.cumiou[i] = 0.f;
        if (pano) t.cumfix[i] = 0;
    }
    if (!pano) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.cap; i += stride) {
        t.pair_key[i] = kSegEmpty; t.gt_key[i] = kSegEmpty; t.pred_key[i] = kSegEmpty;
        t.pair_cnt[i] = 0; t.gt_cnt[i] = 0; t.pred_cnt[i] = 0;
    }
}

// per_wg: points of a workgroup, a multiple of kSegStep; vec: all four arrays 16-byte aligned
__global__ __launch_bounds__(256) void k_seg_points(const uint8_t *__restrict__ gtl, const uint8_t *__restrict__ prl,
                                                    const uint16_t *__restrict__ gti, const uint16_t *__restrict__ pri,
                                                    const int64_t *__restrict__ off, int64_t n, int frames, int64_t per_wg,
                                                    int vec, SegArgs a, SegTables t, SegOut o)
{
    __shared__ u64 skey[kSegLdsSlots];
    __shared__ uint32_t scnt[kSegLdsSlots];
    __shared__ uint32_t smap[256];                           // label -> (key label) << 16 | id mask
    __shared__ int sframe[2];
    const int tid = threadIdx.x;
    for (int s = tid; s < kSegLdsSlots; s += kSegThreads) { skey[s] = kSegEmpty; scnt[s] = 0; }
    {
        const uint32_t in = (a.mask[tid >> 5] >> (tid & 31)) & 1u;
        smap[tid] = in ? ((uint32_t)tid << 16 | (a.pano ? 0xffffu : 0u)) : ((uint32_t)a.background << 16);
    }
    const int64_t lo = (int64_t)blockIdx.x * per_wg, hi = lo + per_wg < n ? lo + per_wg : n;
    if (tid == 0) {
        const int f0 = seg_frame_of(off, lo, 0, frames - 1);
        sframe[0] = f0;
        sframe[1] = seg_frame_of(off, hi - 1, f0, frames - 1);
    }
    __syncthreads();
    const int wf0 = sframe[0], wf1 = sframe[1];
    for (int64_t base = lo + (int64_t)tid * kSegPerLane; base < hi; base += kSegStep) {
        const int cnt = hi - base < kSegPerLane ? (int)(hi - base) : kSegPerLane;
        uint32_t g[kSegPerLane / 4], p[kSegPerLane / 4], ig[kSegPerLane / 2], ip[kSegPerLane / 2];
        if (vec && cnt == kSegPerLane) {
            const uint4 vg = *(const uint4 *)(gtl + base), vp = *(const uint4 *)(prl + base);
            g[0] = vg.x; g[1] = vg.y; g[2] = vg.z; g[3] = vg.w;
            p[0] = vp.x; p[1] = vp.y; p[2] = vp.z; p[3] = vp.w;
            if (a.pano) {
                const uint4 a0 = *(const uint4 *)(gti + base), a1 = *(const uint4 *)(gti + base + 8);
                const uint4 b0 = *(const uint4 *)(pri + base), b1 = *(const uint4 *)(pri + base + 8);
                ig[0] = a0.x; ig[1] = a0.y; ig[2] = a0.z; ig[3] = a0.w; ig[4] = a1.x; ig[5] = a1.y; ig[6] = a1.z; ig[7] = a1.w;
                ip[0] = b0.x; ip[1] = b0.y; ip[2] = b0.z; ip[3] = b0.w; ip[4] = b1.x; ip[5] = b1.y; ip[6] = b1.z; ip[7] = b1.w;
            } else {
#pragma unroll
                for (int j = 0; j < kSegPerLane / 2; j++) { ig[j] = 0; ip[j] = 0; }
            }
        } else {                                             // unaligned views, the tail: byte / short loads, zero padding
#pragma unroll
            for (int j = 0; j < kSegPerLane / 4; j++) { g[j] = 0; p[j] = 0; }
#pragma unroll
            for (int j = 0; j < kSegPerLane / 2; j++) { ig[j] = 0; ip[j] = 0; }
#pragma unroll
            for (int j = 0; j < kSegPerLane; j++)
                if (j < cnt) {
                    g[j >> 2] |= (uint32_t)gtl[base + j] << (8 * (j & 3));
                    p[j >> 2] |= (uint32_t)prl[base + j] << (8 * (j & 3));
                    if (a.pano) {
                        ig[j >> 1] |= (uint32_t)gti[base + j] << (16 * (j & 1));
                        ip[j >> 1] |= (uint32_t)pri[base + j] << (16 * (j & 1));
                    }
                }
        }
        int f = seg_frame_of(off, base, wf0, wf1);
        int64_t next = f + 1 < frames ? off[f + 1] : INT64_MAX;
        u64 run_key = kSegEmpty;
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < kSegPerLane; j++) {
            if (j < cnt) {
                while (base + j >= next) { f++; next = f + 1 < frames ? off[f + 1] : INT64_MAX; }
                const uint32_t mg = smap[(g[j >> 2] >> (8 * (j & 3))) & 0xff];
                const uint32_t mp = smap[(p[j >> 2] >> (8 * (j & 3))) & 0xff];
                const uint32_t gk = (mg & 0xff0000u) | ((ig[j >> 1] >> (16 * (j & 1))) & mg & 0xffffu);
                const uint32_t pk = (mp & 0xff0000u) | ((ip[j >> 1] >> (16 * (j & 1))) & mp & 0xffffu);
                const u64 key = (u64)f << 48 | (u64)gk << 24 | pk;
                if (key == run_key) run++;
                else {
                    if (run) seg_lds_add(skey, scnt, t, o, a, run_key, run);
                    run_key = key;
                    run = 1;
                }
            }
        }
        if (run) seg_lds_add(skey, scnt, t, o, a, run_key, run);
    }
    __syncthreads();
    for (int s = tid; s < kSegLdsSlots; s += kSegThreads) {
        const u64 k = skey[s];
        if (k != kSegEmpty) seg_record(t, o, a, k, scnt[s]);
    }
}

// :1032-1063 over the distinct pairs: a pair is matched when both labels are the same class (not background), its gt key has
// at least min_points points and iou = inter / (g + p - inter) > 0.5 in fp32
__global__ __launch_bounds__(256) void k_seg_match(SegTables t, SegOut o, SegArgs a)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t bg = (uint32_t)a.background;
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap; s += stride) {
        const u64 key = t.pair_key[s];
        if (key == kSegEmpty) continue;
        const uint32_t gl = (uint32_t)(key >> 40) & 0xff, pl = (uint32_t)(key >> 16) & 0xff;
        if (gl == bg || pl == bg || gl != pl) continue;
        const u64 f = key >> 48;
        const u64 gs = seg_global_find(t.gt_key, t.cap, f << 24 | ((key >> 24) & 0xffffff));
        if (gs == t.cap) continue;
        const int64_t gc = (int64_t)(t.gt_cnt[gs] & ~kSegMatched);
        if (gc < a.min_points) continue;
        const u64 ps = seg_global_find(t.pred_key, t.cap, f << 24 | (key & 0xffffff));
        if (ps == t.cap) continue;
        const int64_t pc = (int64_t)(t.pred_cnt[ps] & ~kSegMatched), inter = (int64_t)t.pair_cnt[s];
        const float total = (float)(gc + pc - inter);
        const float iou = (float)inter / total;
        if (iou > 0.5f) {
            atomicAdd(&o.itp[f * 256 + gl], 1);
            atomicAdd(&t.cumfix[f * 256 + gl], (u64)(iou * 16777216.f));
            atomicOr(&t.gt_cnt[gs], kSegMatched);
            atomicOr(&t.pred_cnt[ps], kSegMatched);
        }
    }
}

// :1064-1075: unmatched gt keys -> ifn, unmatched pred keys -> ifp (class keys with at least min_points points); the sums
__global__ __launch_bounds__(256) void k_seg_final(SegTables t, SegOut o, SegArgs a, int64_t fcells)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t bg = (uint32_t)a.background;
    for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap; s += stride) {
        const u64 gk = t.gt_key[s], pk = t.pred_key[s];
        if (gk != kSegEmpty) {
            const uint32_t c = t.gt_cnt[s], l = (uint32_t)(gk >> 16) & 0xff;
            if (l != bg && !(c & kSegMatched) && (int64_t)c >= a.min_points) atomicAdd(&o.ifn[(gk >> 24) * 256 + l], 1);
        }
        if (pk != kSegEmpty) {
            const uint32_t c = t.pred_cnt[s], l = (uint32_t)(pk >> 16) & 0xff;
            if (l != bg && !(c & kSegMatched) && (int64_t)c >= a.min_points) atomicAdd(&o.ifp[(pk >> 24) * 256 + l], 1);
        }
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)fcells; i += stride)
        o.cumiou[i] = (float)((double)t.cumfix[i] * 0x1p-24);
}

u64 seg_cap(int64_t n) { return (u64)d3d_align_up((size_t)(n + n / 4 + 64), 64); }

SegTables seg_carve(WsCarver &w, int64_t n, int64_t frames)
{
    SegTables t;
    t.cap = seg_cap(n);
    t.pair_key = w.take<u64>(t.cap);
    t.gt_key = w.take<u64>(t.cap);
    t.pred_key = w.take<u64>(t.cap);
    t.pair_cnt = w.take<uint32_t>(t.cap);
    t.gt_cnt = w.take<uint32_t>(t.cap);
    t.pred_cnt = w.take<uint32_t>(t.cap);
    t.cumfix = w.take<u64>((size_t)frames * 256);
    return t;
}

unsigned seg_grid(u64 items)
{
    const u64 b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}
}  // namespace

extern "C" size_t d3d_segeval_workspace_bytes(int64_t n, int64_t frames)
{
    if (n < 0 || frames < 0) return 0;
    WsCarver w(nullptr, 0);
    seg_carve(w, n, frames);
    return w.off;
}

extern "C" int d3d_segeval(const uint8_t *gt_labels, const uint8_t *pred_labels, const uint16_t *gt_ids, const uint16_t *pred_ids,
                           const int64_t *frame_off, int64_t n, int64_t frames, const uint32_t *class_mask,
                           int32_t background, int32_t min_points,
                           int32_t *tp, int32_t *fp, int32_t *fn, int32_t *itp, int32_t *ifp, int32_t *ifn, float *cumiou,
                           void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || frames < 0 || frames > 65535 || n >= ((int64_t)1 << 31) || !class_mask) return D3D_ERR_BAD_ARG;
    if (background < 0 || background > 255) return D3D_ERR_BAD_ARG;
    if ((gt_ids == nullptr) != (pred_ids == nullptr)) return D3D_ERR_BAD_ARG;
    if (n > 0 && (frames == 0 || !gt_labels || !pred_labels || !frame_off)) return D3D_ERR_BAD_ARG;
    if (frames == 0) return D3D_OK;
    if (!tp || !fp || !fn || !itp || !ifp || !ifn || !cumiou) return D3D_ERR_BAD_ARG;
    WsCarver w(workspace, workspace_bytes);
    SegTables t = seg_carve(w, n, frames);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    SegArgs a;
    for (int k = 0; k < 8; k++) a.mask[k] = class_mask[k];
    a.background = background;
    a.min_points = min_points;
    a.pano = gt_ids != nullptr;
    SegOut o{tp, fp, fn, itp, ifp, ifn, cumiou};
    const int64_t fcells = frames * 256;
    D3D_LAUNCH("k_seg_init", k_seg_init, dim3(seg_grid(a.pano ? (t.cap > (u64)fcells ? t.cap : (u64)fcells) : (u64)fcells)),
               dim3(256), 0, st, t, o, fcells, a.pano);
    if (n > 0) {
        const int64_t steps = d3d_divup(n, kSegStep);
        const int64_t blocks = steps < kSegMaxBlocks ? steps : kSegMaxBlocks;
        const int64_t per_wg = d3d_divup(steps, blocks) * kSegStep;
        const int vec = ((reinterpret_cast<uintptr_t>(gt_labels) | reinterpret_cast<uintptr_t>(pred_labels) |
                          reinterpret_cast<uintptr_t>(gt_ids) | reinterpret_cast<uintptr_t>(pred_ids)) & 15) == 0;
        D3D_LAUNCH("k_seg_points", k_seg_points, dim3((unsigned)d3d_divup(n, per_wg)), dim3(kSegThreads), 0, st,
                   gt_labels, pred_labels, gt_ids, pred_ids, frame_off, n, (int)frames, per_wg, vec, a, t, o);
    }
    if (a.pano) {
        if (n > 0) D3D_LAUNCH("k_seg_match", k_seg_match, dim3(seg_grid(t.cap)), dim3(256), 0, st, t, o, a);
        D3D_LAUNCH("k_seg_final", k_seg_final, dim3(seg_grid(t.cap > (u64)fcells ? t.cap : (u64)fcells)), dim3(256), 0, st,
                   t, o, a, fcells);
    }
    return D3D_OK;
}
