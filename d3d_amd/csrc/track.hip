// track.hip -- TrackingEvaluator.calc_stats of the reference (d3d/benchmarks.pyx:536-723) for one frame, all score thresholds.
//
// The reference walks, per frame and per threshold, the carried-over assignments of the previous frame (hash maps of 64-bit
// track ids), runs a ScoreMatcher on what is left and walks three more hash maps for the id switches, the fragments and the
// next frame's state.  Here the state lives on the device, so a frame is a chain of launches without a host round trip:
//
//   k_track_prepare  workgroups 0 .. T-1: one per threshold.  The selected detections (`score < thres` skips, :590-593); the
//                    carried pairs of the state, each looked up by tid in the frame (binary search in the host-sorted
//                    (tid, row) tables: first hit among ALL gt rows, :602-614) and tested against the distance cache (`>`
//                    rematches, :605); the subset that goes to the matcher in index order (the rows whose distances the k-th
//                    slot walks, matcher.pyx:155-158) and in score order (the k-th best: whose acceptable pairs it takes),
//                    written as the row / mask indices of d3d_score_match_batched.  Slots of selected detections that stay out
//                    of the subset are padding at the end of the problem: they read the all-zero mask row and take nothing.
//                    Workgroups T ..: the acceptable-pair mask [(n + 1), m] (tag, the detection's own distance within the
//                    ground truth's threshold; row n = zeros) and the matcher's neutral column arrays.
//   d3d_score_match_batched  unchanged: the literal association of every threshold, one problem each.
//   k_track_update   one workgroup per threshold: the overwrite rule (:622-635), the assignment of every ground truth, fp
//                    (:660-665), id switches and fragments against the previous state (:672-689), the next state (:691-707).
//
// State (double-buffered by the caller): per threshold a count and up to `capacity` pairs (gt_tid, dt_tid, gt_class,
// dt_class) -- the reference's _last_gt_assignment / _last_dt_assignment / _last_*_tags, which are one bijection when the tids
// of a frame are unique (the caller rejects frames where they are not).  Classes are slots 0 .. C-1 of the evaluator's class
// list, -1 = outside it (counts under such a class are dropped).
#include "common.hpp"

namespace {
typedef uint64_t u64;

constexpr int kTrackThreads = 256;
constexpr int kTrackWaves = kTrackThreads / kWave;
constexpr int kMaskBlocks = 1024;
// status of a detection at a threshold (prepare -> update)
constexpr int8_t kNotSelected = 0, kSubset = 1, kKeptCarry = 2, kCarryAbsent = 3;

struct TrackState {
    int32_t *count;          // [T]
    u64 *gt_tid, *dt_tid;    // [T, cap]
    int32_t *gt_cls, *dt_cls;
};

TrackState state_carve(WsCarver &w, int64_t cap, int T)
{
    TrackState s;
    s.count = w.take<int32_t>((size_t)T);
    s.gt_tid = w.take<u64>((size_t)T * (size_t)cap);
    s.dt_tid = w.take<u64>((size_t)T * (size_t)cap);
    s.gt_cls = w.take<int32_t>((size_t)T * (size_t)cap);
    s.dt_cls = w.take<int32_t>((size_t)T * (size_t)cap);
    return s;
}

struct TrackScratch {
    int8_t *status;          // [T, n]
    int32_t *kept_det;       // [T, m]: the carried detection kept on ground truth j, -1
    int32_t *det_gt;         // [T, n]: the ground truth assigned to detection d (update), -1
    int64_t *row_src, *row_mask, *order;   // [n_total]
    int32_t *src_tag0;       // [n_total]
    int32_t *dst_tag0;       // [m]
    float *dst_thr;          // [m]
    uint8_t *mask;           // [(n + 1), m]
    int32_t *src_match;      // [n_total]
    int32_t *dst_match;      // [T, m]
    int32_t *status_word;
    void *match_ws;
    size_t match_ws_bytes;
};

TrackScratch scratch_carve(WsCarver &w, int64_t n, int64_t m, int T, int64_t n_total)
{
    TrackScratch s;
    s.status = w.take<int8_t>((size_t)T * (size_t)n);
    s.kept_det = w.take<int32_t>((size_t)T * (size_t)m);
    s.det_gt = w.take<int32_t>((size_t)T * (size_t)n);
    s.row_src = w.take<int64_t>((size_t)n_total);
    s.row_mask = w.take<int64_t>((size_t)n_total);
    s.order = w.take<int64_t>((size_t)n_total);
    s.src_tag0 = w.take<int32_t>((size_t)n_total);
    s.dst_tag0 = w.take<int32_t>((size_t)m);
    s.dst_thr = w.take<float>((size_t)m);
    s.mask = w.take<uint8_t>((size_t)(n + 1) * (size_t)m);
    s.src_match = w.take<int32_t>((size_t)n_total);
    s.dst_match = w.take<int32_t>((size_t)T * (size_t)m);
    s.status_word = w.take<int32_t>(1);
    s.match_ws_bytes = d3d_score_match_batched_workspace_bytes(n_total, m, T);
    s.match_ws = w.take<uint8_t>(s.match_ws_bytes);
    return s;
}

// row of `tid` in a frame's sorted (tid, row) table, -1 if absent
__device__ __forceinline__ int32_t find_row(const u64 *__restrict__ stid, const int32_t *__restrict__ srow, int64_t len, u64 tid)
{
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (stid[mid] < tid) lo = mid + 1; else hi = mid;
    }
    return (lo < len && stid[lo] == tid) ? srow[lo] : -1;
}

// stream compaction inside one workgroup: the exclusive rank of this thread's flag among the flags of the whole 256-thread
// step, and the step's total (the same in every thread).  Two barriers; `wtot` holds kTrackWaves ints of LDS.
__device__ __forceinline__ int block_rank(bool flag, int *wtot, int &total)
{
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const unsigned long long b = __ballot(flag);
    const int in_wave = __popcll(b & ((1ull << lane) - 1));
    if (lane == 0) wtot[w] = __popcll(b);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < kTrackWaves; k++) {
        const int v = wtot[k];
        base += k < w ? v : 0;
        total += v;
    }
    __syncthreads();
    return base + in_wave;
}

__device__ __forceinline__ bool selected(const float *__restrict__ boxes, const int32_t *__restrict__ cls, int64_t d, float thr)
{
    return cls[d] >= 0 && !(boxes[d * 9 + 1] < thr);
}

__global__ __launch_bounds__(kTrackThreads) void k_track_prepare(D3DTrackFrame f, const float *__restrict__ thresholds, int T,
                                                                 const float *__restrict__ max_dist, TrackState in,
                                                                 TrackScratch s)
{
    const int64_t n = f.n, m = f.m;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= T) {                               // the acceptable-pair mask and the neutral column arrays
        const int64_t first = (int64_t)(blockIdx.x - T) * kTrackThreads + tid, stride = (int64_t)(gridDim.x - T) * kTrackThreads;
        for (int64_t j = first; j < m; j += stride) { s.dst_tag0[j] = 0; s.dst_thr[j] = 3.0e38f; }
        const int64_t cells = (n + 1) * m;
        for (int64_t e = first; e < cells; e += stride) {
            const int64_t r = e / m, j = e - r * m;
            uint8_t ok = 0;
            if (r < n) {
                const int32_t gc = f.gt_cls[j];
                ok = gc >= 0 && f.dt_cls[r] == gc && f.cache[e] <= max_dist[gc];
            }
            s.mask[e] = ok;
        }
        return;
    }
    __shared__ int wtot[kTrackWaves];
    const int t = blockIdx.x;
    const float thr = thresholds[t];
    int8_t *status = s.status + (int64_t)t * n;
    int32_t *kept = s.kept_det + (int64_t)t * m;
    for (int64_t d = tid; d < n; d += kTrackThreads) status[d] = selected(f.dt_boxes, f.dt_cls, d, thr) ? kSubset : kNotSelected;
    for (int64_t j = tid; j < m; j += kTrackThreads) kept[j] = -1;
    __syncthreads();
    // carried pairs (:599-614): a selected detection with a previous assignment keeps it when its previous ground truth is in
    // the frame within the distance; is matched afresh when that ground truth is farther; takes no part when it is absent
    const int32_t cnt = in.count[t];
    for (int32_t p = tid; p < cnt; p += kTrackThreads) {
        const int64_t q = (int64_t)t * f.capacity + p;
        const int32_t r = find_row(f.dt_stid, f.dt_srow, n, in.dt_tid[q]);
        if (r < 0 || status[r] == kNotSelected) continue;
        const int32_t g = find_row(f.gt_stid, f.gt_srow, m, in.gt_tid[q]);
        if (g < 0) status[r] = kCarryAbsent;
        else if (!(f.cache[(int64_t)r * m + g] > max_dist[f.dt_cls[r]])) { status[r] = kKeptCarry; kept[g] = r; }
    }
    __syncthreads();
    const int64_t off = f.row_off[t], rows = f.row_off[t + 1] - off;
    // the subset in index order (dt_indices, :601 / :606) and in score order (np.flip(np.argsort(.)), the host's permutation)
    int64_t k = 0;
    for (int64_t d0 = 0; d0 < n; d0 += kTrackThreads) {
        const int64_t d = d0 + tid;
        const bool in_sub = d < n && status[d] == kSubset;
        int total;
        const int rank = block_rank(in_sub, wtot, total);
        if (in_sub && k + rank < rows) s.row_src[off + k + rank] = d;
        k += total;
    }
    k = 0;
    for (int64_t i0 = 0; i0 < n; i0 += kTrackThreads) {
        const int64_t i = i0 + tid;
        const int32_t d = i < n ? f.dt_perm[i] : 0;
        const bool in_sub = i < n && status[d] == kSubset;
        int total;
        const int rank = block_rank(in_sub, wtot, total);
        if (in_sub && k + rank < rows) s.row_mask[off + k + rank] = d;
        k += total;
    }
    for (int64_t r = tid; r < rows; r += kTrackThreads) {
        s.order[off + r] = r;
        if (r >= k) { s.row_src[off + r] = 0; s.row_mask[off + r] = n; }      // padding: the all-zero mask row
    }
}

__global__ __launch_bounds__(kTrackThreads) void k_track_update(D3DTrackFrame f, const float *__restrict__ thresholds, int T,
                                                                int C, TrackState in, TrackState out, TrackScratch s,
                                                                int32_t *assign, float *iou, int32_t *counts)
{
    extern __shared__ int cnt_l[];                           // [3][C]: fp, id switches, fragments
    __shared__ int wtot[kTrackWaves];
    const int64_t n = f.n, m = f.m;
    const int tid = threadIdx.x, t = blockIdx.x;
    const int8_t *status = s.status + (int64_t)t * n;
    const int32_t *kept = s.kept_det + (int64_t)t * m;
    const int32_t *dm = s.dst_match + (int64_t)t * m;
    int32_t *det_gt = s.det_gt + (int64_t)t * n;
    int32_t *asg = assign + (int64_t)t * m;
    const int64_t off = f.row_off[t], rows = f.row_off[t + 1] - off;
    for (int k = tid; k < 3 * C; k += kTrackThreads) cnt_l[k] = 0;
    for (int64_t d = tid; d < n; d += kTrackThreads) det_gt[d] = -1;
    __syncthreads();
    // every ground truth's detection (:617-635): a fresh match overwrites a kept carry-over, counted as fp of the NEW detection
    for (int64_t j = tid; j < m; j += kTrackThreads) {
        const int32_t slot = dm[j];
        const int64_t pick = (slot >= 0 && slot < rows) ? s.row_mask[off + slot] : -1;
        const int32_t fresh = pick < n ? (int32_t)pick : -1;             // (padding slots read row n: they never match)
        const int32_t carried = kept[j];
        if (fresh >= 0 && carried >= 0) atomicAdd(&cnt_l[f.dt_cls[fresh]], 1);
        const int32_t a = fresh >= 0 ? fresh : carried;
        asg[j] = a;
        iou[(int64_t)t * m + j] = a >= 0 ? 1.0f - f.cache[(int64_t)a * m + j] : 0.0f;
        if (a >= 0) det_gt[a] = (int32_t)j;
    }
    __syncthreads();
    for (int64_t d = tid; d < n; d += kTrackThreads)                          // :660-665
        if (status[d] == kSubset && det_gt[d] < 0) atomicAdd(&cnt_l[f.dt_cls[d]], 1);
    const int32_t cnt = in.count[t];
    for (int32_t p = tid; p < cnt; p += kTrackThreads) {                        // :672-689
        const int64_t q = (int64_t)t * f.capacity + p;
        const u64 gtid = in.gt_tid[q], dtid = in.dt_tid[q];
        const int32_t gc = in.gt_cls[q], dc = in.dt_cls[q];
        const int32_t g = find_row(f.gt_stid, f.gt_srow, m, gtid);
        const int32_t a = g >= 0 ? asg[g] : -1;
        const bool sw = a < 0 ? (g >= 0 && f.gt_cls[g] >= 0) : f.dt_tid[a] != dtid;
        if (sw && gc >= 0) atomicAdd(&cnt_l[C + gc], 1);
        const int32_t r = find_row(f.dt_stid, f.dt_srow, n, dtid);
        const int32_t ga = r >= 0 ? det_gt[r] : -1;
        const bool fr = ga < 0 ? (r >= 0 && status[r] != kNotSelected) : f.gt_tid[ga] != gtid;
        if (fr && dc >= 0) atomicAdd(&cnt_l[2 * C + dc], 1);
    }
    // the next state (:691-707): one pair per assigned ground truth, in row order
    int64_t k = 0;
    for (int64_t j0 = 0; j0 < m; j0 += kTrackThreads) {
        const int64_t j = j0 + tid;
        const int32_t a = j < m ? asg[j] : -1;
        int total;
        const int rank = block_rank(a >= 0, wtot, total);
        if (a >= 0 && k + rank < f.capacity) {
            const int64_t q = (int64_t)t * f.capacity + k + rank;
            out.gt_tid[q] = f.gt_tid[j];
            out.dt_tid[q] = f.dt_tid[a];
            out.gt_cls[q] = f.gt_cls[j];
            out.dt_cls[q] = f.dt_cls[a];
        }
        k += total;
    }
    if (tid == 0) out.count[t] = (int32_t)(k < f.capacity ? k : f.capacity);
    __syncthreads();
    for (int k2 = tid; k2 < 3 * C; k2 += kTrackThreads) counts[(int64_t)t * 3 * C + k2] = cnt_l[k2];
}
}  // namespace

extern "C" size_t d3d_track_state_bytes(int64_t capacity, int32_t thresholds)
{
    if (capacity < 0 || thresholds < 1) return 0;
    WsCarver w(nullptr, 0);
    state_carve(w, capacity, thresholds);
    return w.off;
}

extern "C" size_t d3d_track_workspace_bytes(int64_t n, int64_t m, int32_t thresholds, int64_t n_total)
{
    if (n < 0 || m < 0 || thresholds < 1 || n_total < 0) return 0;
    WsCarver w(nullptr, 0);
    scratch_carve(w, n, m, thresholds, n_total);
    return w.off + 256;
}

extern "C" int d3d_track_frame(const D3DTrackFrame *frame, const float *thresholds, int32_t T, const float *max_dist,
                               int32_t C, const void *state_in, void *state_out, int32_t *assign, float *iou, int32_t *counts,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!frame || T < 1 || T > 65535 || C < 1 || C > 4096 || !thresholds || !max_dist || !state_in || !state_out ||
        state_in == state_out || !counts)
        return D3D_ERR_BAD_ARG;
    const D3DTrackFrame &f = *frame;
    const int64_t n = f.n, m = f.m, n_total = f.n_total;
    if (n < 0 || m < 0 || n_total < 0 || n_total > n * (int64_t)T || f.capacity < m || n >= (1ll << 31) || m >= (1ll << 31))
        return D3D_ERR_BAD_ARG;
    if ((n > 0 && (!f.dt_boxes || !f.dt_cls || !f.dt_tid || !f.dt_stid || !f.dt_srow || !f.dt_perm)) ||
        (m > 0 && (!f.gt_cls || !f.gt_tid || !f.gt_stid || !f.gt_srow || !assign || !iou)) ||
        (n > 0 && m > 0 && !f.cache) || !f.row_off)
        return D3D_ERR_BAD_ARG;
    WsCarver w(workspace, workspace_bytes);
    TrackScratch s = scratch_carve(w, n, m, T, n_total);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    WsCarver wi((void *)state_in, d3d_track_state_bytes(f.capacity, T)), wo(state_out, d3d_track_state_bytes(f.capacity, T));
    const TrackState in = state_carve(wi, f.capacity, T), out = state_carve(wo, f.capacity, T);
    const int64_t cells = (n + 1) * m;
    const int64_t mask_blocks = cells > 0 ? (d3d_divup(cells, kTrackThreads) < kMaskBlocks ? d3d_divup(cells, kTrackThreads) : kMaskBlocks) : 0;
    D3D_LAUNCH("k_track_prepare", k_track_prepare, dim3((unsigned)(T + mask_blocks)), dim3(kTrackThreads), 0, st, f, thresholds, T,
               max_dist, in, s);
    if (n_total > 0) D3D_HIP_CHECK(hipMemsetAsync(s.src_tag0, 0, (size_t)n_total * 4, st));
    if (m > 0) {
        const int rc = d3d_score_match_batched(f.cache, s.row_src, s.mask, s.row_mask, f.row_off, T, n_total, m, s.src_tag0,
                                               s.dst_tag0, s.dst_thr, s.order, s.src_match, s.dst_match, s.status_word, s.match_ws,
                                               s.match_ws_bytes, stream);
        if (rc != D3D_OK) return rc;
    }
    D3D_LAUNCH("k_track_update", k_track_update, dim3((unsigned)T), dim3(kTrackThreads), (size_t)3 * C * sizeof(int), st, f,
               thresholds, T, C, in, out, s, assign, iou, counts);
    return D3D_OK;
}
