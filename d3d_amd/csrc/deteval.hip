// deteval.hip -- DetectionEvaluator.calc_stats (reference d3d/benchmarks.pyx:188-283) for MANY frames in one call.  An
// extension: the reference evaluates one frame per call, and so do d3d_match_distance + d3d_score_match_batched, whose
// problems share one destination set.  A validation split is thousands of frames of a few dozen to a few hundred boxes: the
// arithmetic is microseconds, the per-frame launches and waits are the cost.  Two launches serve a whole chunk of frames:
//
//   k_deteval_distance  the ragged distance cache (BaseMatcher.prepare_boxes, matcher.pyx:24-82, RIoU): one lane per
//                       (detection, ground truth) pair of ANY frame; the lane finds its frame by bisection over the frames' cache
//                       offsets and runs the per-pair fp32 recipe of k_iou3d_paired / k_iou3d_small (geom.hpp) on the rows
//                       with their dimensions clipped to +-1e3, so an entry has d3d_match_distance's bits.
//   k_deteval_assoc     the association (ScoreMatcher.match, matcher.pyx:142-162 over match_by_order, :90-121): ONE wavefront
//                       per problem -- per (frame, score threshold) for the reference's literal pairing, per frame for the
//                       own-row pairing -- walks the slots in order.  For a slot the 64 lanes sweep the frame's ground truths
//                       (the slot's two cache rows come from L2, coalesced), keep the nearest acceptable free one per lane, and
//                       a wave reduction picks the winner, ties to the lower ground-truth index.  The "free" state is the LDS
//                       copy of the ground truths' classes (taken = -1); no global atomics, no workspace, nothing waits on
//                       another workgroup.  Problems this small do not pay for match.hip's candidate lists and deferred
//                       acceptance (three launches and 512 B of lists per row).  4 KB of LDS per wavefront keeps all 32 wave
//                       slots of a CU resident (a 200 x 50 frame's cache staged in LDS, 40 KB, would leave four), which is
//                       what hides the L2 latency of a serial walk; a frame's thresholds read the same rows.
//
// The literal pairing (ReferenceAssociation in d3d_amd/tracking/matcher.py restates matcher.pyx:155-158): slot k of a threshold
// ACCEPTS the ground truths of the k-th best selected detection (its class, ITS distance within the class threshold) but
// PREFERS them in the distance order of the k-th selected detection in index order -- another box unless the detections are
// already sorted by score.  The host hands over, per frame, the in-class detections in score order (every threshold's selection
// is a prefix of it) and every detection's position in that order; the selected detections in index order are then those with
// a position below the threshold's count, compacted by ballot into LDS.
#include "common.hpp"
#include "geom.hpp"
#include <math.h>

namespace {

constexpr int kDetFrameMax = 1024;      // boxes of one frame on either side (see d3d_deteval_frame_max)
constexpr int kDistLanes = 256;

struct Row3D {
    BoxGeom<float> g;
    float zmin, zmax;
};

// a [.,9] row (label, score, x, y, z, lx, ly, lz, yaw) as box.hip's load3d(row + 2, clip_dims = true) builds it
__device__ __forceinline__ Row3D load_row(const float *__restrict__ b)
{
    const float lx = fminf(fmaxf(b[5], -1e3f), 1e3f), ly = fminf(fmaxf(b[6], -1e3f), 1e3f), lz = fminf(fmaxf(b[7], -1e3f), 1e3f);
    Row3D r;
    r.g = make_geom<float>(b[2], b[3], lx, ly, b[8]);
    r.zmax = b[4] + lz / 2;
    r.zmin = b[4] - lz / 2;
    return r;
}

struct DetFrames {
    const float *dt, *gt;                          // [N,9], [M,9]: the frames' rows stacked
    const int64_t *dt_off, *gt_off, *cache_off;    // [frames + 1] each
    int64_t frames;
};

__global__ __launch_bounds__(kDistLanes) void k_deteval_distance(DetFrames fr, float *__restrict__ cache)
{
    const int64_t p = (int64_t)blockIdx.x * kDistLanes + threadIdx.x;
    if (p >= fr.cache_off[fr.frames]) return;
    int64_t lo = 0, hi = fr.frames;                 // the last frame whose cache starts at or before p (empty ones start where the
    while (hi - lo > 1) {                           // next one does and are passed over)
        const int64_t mid = (lo + hi) >> 1;
        if (fr.cache_off[mid] <= p) lo = mid; else hi = mid;
    }
    const int64_t g0 = fr.gt_off[lo], m = fr.gt_off[lo + 1] - g0, q = p - fr.cache_off[lo];
    if (m <= 0) return;                                       // (offsets that do not describe n x m caches: nothing out of a frame)
    const int64_t i = q / m, j = q - i * m;
    if (i >= fr.dt_off[lo + 1] - fr.dt_off[lo]) return;
    const Row3D a = load_row(fr.dt + (fr.dt_off[lo] + i) * 9), b = load_row(fr.gt + (g0 + j) * 9);
    float v = 0.f;
    if (aabb_gap(cand_aabb(a.g, true), cand_aabb(b.g, true)) > 0.f) {
        const float bev = iou_rbox(a.g, b.g);
        if (bev != 0.f) {
            const float imax = fminf(a.zmax, b.zmax), imin = fmaxf(a.zmin, b.zmin);
            const float umax = fmaxf(a.zmax, b.zmax), umin = fminf(a.zmin, b.zmin);
            v = bev * (fmaxf(imax - imin, 0.f) / fmaxf(umax - umin, (float)1e-6));
        }
    }
    cache[p] = 1 - v;
}

__device__ __forceinline__ bool pair_less(float d1, int j1, float d2, int j2) { return d1 < d2 || (d1 == d2 && j1 < j2); }

struct DetAssoc {
    const int32_t *dt_cls, *gt_cls;     // [N], [M]: class slots 0 .. C-1, negative = outside the evaluated classes
    const int32_t *dt_perm;             // [N]: frame f's in-class detections in score order (local rows) at dt_off[f] ..
    const int32_t *dt_rank;             // [N]: a detection's position in that order, negative = outside the classes
    const int32_t *slots;               // [problems]: the slots of a problem = the detections it walks
    const float *max_dist;              // [C]
    const float *cache;
    int32_t *gt_match;                  // [problems' ground truths]: the detection (local row) or -1
    float *gt_iou;                      // the same layout: 1 - cache of the pair, 0 without one
    int32_t *dt_match;                  // [N], own-row pairing only: the ground truth (local row) or -1
    int32_t T;
};

template <bool LITERAL>
__global__ __launch_bounds__(kWave) void k_deteval_assoc(DetFrames fr, DetAssoc s)
{
    __shared__ int16_t free_cls[kDetFrameMax];       // a ground truth's class while it is free, -1 once taken (or outside)
    __shared__ uint16_t by_index[kDetFrameMax];      // LITERAL: the selected detections in index order
    const int lane = threadIdx.x;
    const int64_t prob = blockIdx.x, f = LITERAL ? prob / s.T : prob;
    const int t = LITERAL ? (int)(prob - f * s.T) : 0;
    const int64_t d0 = fr.dt_off[f], g0 = fr.gt_off[f];
    const int64_t n64 = fr.dt_off[f + 1] - d0, m64 = fr.gt_off[f + 1] - g0;
    if (n64 > kDetFrameMax || m64 > kDetFrameMax || n64 < 0 || m64 < 0) return;      // (the entry refuses such a batch)
    const int n = (int)n64, m = (int)m64;
    const int64_t ob = LITERAL ? (int64_t)s.T * g0 + (int64_t)t * m : g0;
    for (int j = lane; j < m; j += kWave) {
        s.gt_match[ob + j] = -1;
        s.gt_iou[ob + j] = 0.f;
        const int32_t c = s.gt_cls[g0 + j];
        free_cls[j] = (int16_t)(c < 0 ? -1 : c);
    }
    if (!LITERAL)
        for (int d = lane; d < n; d += kWave) s.dt_match[d0 + d] = -1;
    int K = s.slots[prob];
    if (K > n) K = n;
    if (LITERAL) {
        int k = 0;
        for (int c0 = 0; c0 < n; c0 += kWave) {
            const int d = c0 + lane;
            const int32_t r = d < n ? s.dt_rank[d0 + d] : -1;
            const bool in = r >= 0 && r < K;
            const unsigned long long b = __ballot(in);
            if (in) by_index[k + __popcll(b & ((1ull << lane) - 1))] = (uint16_t)d;
            k += __popcll(b);
        }
        if (K > k) K = k;
    }
    __syncthreads();
    if (m == 0) return;
    const float *__restrict__ cache = s.cache + fr.cache_off[f];
    for (int k0 = 0; k0 < K; k0 += kWave) {
        // 64 slots' detections and classes at a time: one load each, handed round by lane broadcasts
        const int kk = k0 + lane;
        const int32_t my_a = kk < K ? s.dt_perm[d0 + kk] : 0;
        const int32_t my_c = kk < K ? s.dt_cls[d0 + my_a] : -1;
        const int rows = K - k0 < kWave ? K - k0 : kWave;
        for (int q = 0; q < rows; q++) {
            const int a = __shfl(my_a, q, kWave), ca = __shfl(my_c, q, kWave);
            if (ca < 0) continue;
            const int r = LITERAL ? (int)by_index[k0 + q] : a;
            const float thr = s.max_dist[ca];
            const float *__restrict__ own = cache + (int64_t)a * m, *__restrict__ pref = cache + (int64_t)r * m;
            float bd = INFINITY;
            int bj = 0x7fffffff;
            for (int j = lane; j < m; j += kWave) {
                if (free_cls[j] != ca) continue;
                const float da = own[j], dr = LITERAL ? pref[j] : da;
                // (the literal route hands match_by_order +inf for a pair that is not acceptable and takes entries up to 3e38)
                if (!(da <= thr) || (LITERAL && !(dr <= 3.0e38f))) continue;
                if (pair_less(dr, j, bd, bj)) { bd = dr; bj = j; }
            }
            const unsigned long long have = __ballot(bj != 0x7fffffff);
            if (!have) continue;
            if (have & (have - 1)) {
#pragma unroll
                for (int o = kWave / 2; o > 0; o >>= 1) {
                    const float od = __shfl_xor(bd, o, kWave);
                    const int oj = __shfl_xor(bj, o, kWave);
                    if (pair_less(od, oj, bd, bj)) { bd = od; bj = oj; }
                }
            } else {
                bj = __shfl(bj, __ffsll((long long)have) - 1, kWave);
            }
            if (lane == 0) {
                free_cls[bj] = -1;
                s.gt_match[ob + bj] = a;
                s.gt_iou[ob + bj] = 1.0f - own[bj];
                if (!LITERAL) s.dt_match[d0 + a] = bj;
            }
            __syncthreads();                             // (one wavefront: orders the LDS store before the next slot's reads)
        }
    }
}

// the workspace holds the ragged cache when the caller does not ask for it
struct DetWs {
    float *cache;
};
DetWs det_carve(WsCarver &w, int64_t pairs, bool own_cache)
{
    DetWs c;
    c.cache = w.take<float>(own_cache ? (size_t)pairs : 0);
    return c;
}

}  // namespace

extern "C" int32_t d3d_deteval_frame_max(void) { return kDetFrameMax; }

extern "C" size_t d3d_deteval_batched_workspace_bytes(int64_t pairs, int32_t cache_given)
{
    WsCarver w(nullptr, 0);
    det_carve(w, pairs < 0 ? 0 : pairs, cache_given == 0);
    return w.off;
}

extern "C" int d3d_deteval_batched(const float *dt_boxes, const float *gt_boxes, const int64_t *dt_off, const int64_t *gt_off,
                                   const int64_t *cache_off, int64_t frames, int64_t pairs, int64_t max_n, int64_t max_m,
                                   const int32_t *dt_cls, const int32_t *gt_cls, const int32_t *dt_perm, const int32_t *dt_rank,
                                   const int32_t *slots, int32_t T, const float *max_dist, int32_t C, int32_t literal,
                                   float *cache, int32_t *gt_match, float *gt_iou, int32_t *dt_match,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (frames < 0 || pairs < 0 || max_n < 0 || max_m < 0 || T < 1 || T > 65535 || C < 1 || C > 32767) return D3D_ERR_BAD_ARG;
    if (max_n > kDetFrameMax || max_m > kDetFrameMax) return D3D_ERR_UNSUPPORTED;
    if (frames == 0) return D3D_OK;
    const int64_t problems = frames * (literal ? (int64_t)T : 1);
    if (!dt_off || !gt_off || !cache_off || !slots || !max_dist || problems > 0x7fffffffll ||
        pairs > frames * (int64_t)kDetFrameMax * kDetFrameMax || d3d_divup(pairs, kDistLanes) > 0x7fffffffll)
        return D3D_ERR_BAD_ARG;
    if ((max_n > 0 && (!dt_boxes || !dt_cls || !dt_perm || !dt_rank || (!literal && !dt_match))) ||
        (max_m > 0 && (!gt_boxes || !gt_cls || !gt_match || !gt_iou)))
        return D3D_ERR_BAD_ARG;
    WsCarver w(workspace, workspace_bytes);
    const DetWs c = det_carve(w, pairs, cache == nullptr);
    if (!cache) {
        if (pairs > 0 && (!workspace || !w.ok())) return D3D_ERR_WORKSPACE;
        cache = c.cache;
    }
    const DetFrames fr{dt_boxes, gt_boxes, dt_off, gt_off, cache_off, frames};
    if (pairs > 0)
        D3D_LAUNCH("k_deteval_distance", k_deteval_distance, dim3((unsigned)d3d_divup(pairs, kDistLanes)), dim3(kDistLanes), 0, st, fr, cache);
    const DetAssoc s{dt_cls, gt_cls, dt_perm, dt_rank, slots, max_dist, cache, gt_match, gt_iou, dt_match, T};
    return dispatch(literal != 0, [&](auto lit) {
        D3D_LAUNCH(lit ? "k_deteval_assoc<literal>" : "k_deteval_assoc", k_deteval_assoc<lit>, dim3((unsigned)problems), dim3(kWave), 0, st, fr, s);
        return D3D_OK;
    });
}
