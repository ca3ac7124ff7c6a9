/*
 * d3d_hip.h -- C ABI of libd3d_hip.so: the MI355X (gfx950) implementation of the
 * data-parallel hot path of cmpute/d3d (d3d/voxel + d3d/box, and the operator packages around them: d3d/point, d3d/math).
 *
 * This is the drop-in boundary.  Every entry point replaces one function that the
 * reference binds through pybind11 in d3d/voxel/impl.cpp:3-21 and d3d/box/impl.cpp:8-54
 * (or, for iou3d, the C shims in d3d/dgal_wrap.h reached from Cython).  Conventions:
 *
 *  - plain pointers + sizes, no torch / pybind types;
 *  - all tensor arguments are DEVICE pointers (HBM), contiguous row-major, unless
 *    the parameter comment says "host";
 *  - the caller owns every buffer, including the scratch `workspace` whose size is
 *    returned by the matching *_workspace_bytes() query (256-byte aligned base);
 *  - variable-size results are written into caller-provided upper-bound buffers; the
 *    actual sizes go to a small device array `counts` (int64) that the caller copies
 *    back when it needs them.  No entry point synchronises the stream, allocates,
 *    or touches the legacy default stream (cf. reference nms_cuda.cu:186-214);
 *  - every function returns a d3d_status (0 = ok, <0 = error) instead of throwing
 *    py::value_error or exit()-ing (reference common.h:33-46);
 *  - `stream` is a hipStream_t passed as void* (NULL = null stream).
 */
#ifndef D3D_HIP_H
#define D3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    D3D_OK = 0,
    D3D_ERR_BAD_ARG = -1,       /* null pointer / negative size / bad enum       -> ValueError   */
    D3D_ERR_UNSUPPORTED = -2,   /* option the reference rejects too              -> ValueError   */
    D3D_ERR_WORKSPACE = -3,     /* workspace smaller than *_workspace_bytes()    -> RuntimeError */
    D3D_ERR_HIP = -4            /* a HIP call failed; see d3d_last_hip_error()   -> RuntimeError */
} d3d_status;

/* enum values are the reference's (d3d/voxel/voxelize.h:5-7, d3d/box/common.h:5-10) */
enum { D3D_REDUCE_NONE = 0, D3D_REDUCE_MEAN = 1, D3D_REDUCE_MAX = 2, D3D_REDUCE_MIN = 3 };
enum { D3D_MAXPTS_NONE = 0, D3D_MAXPTS_TRIM = 1, D3D_MAXPTS_FARTHEST_SAMPLING = 2 };
enum { D3D_MAXVOX_NONE = 0, D3D_MAXVOX_TRIM = 1, D3D_MAXVOX_DESCENDING = 2 };
enum { D3D_IOU_NA = 0, D3D_IOU_BOX = 1, D3D_IOU_RBOX = 2, D3D_IOU_GBOX = 3, D3D_IOU_GRBOX = 4,
       D3D_IOU_DBOX = 5, D3D_IOU_DRBOX = 6 };
enum { D3D_SUPPRESS_HARD = 0, D3D_SUPPRESS_LINEAR = 1, D3D_SUPPRESS_GAUSSIAN = 2 };
enum { D3D_F32 = 0, D3D_F64 = 1,
       /* d3d_iou2d_forward / d3d_iou2d_backward, BOX and RBOX only: boxes and box gradients f64, arithmetic f64, the [n,m] MATRIX
        * (ious written, grad read) f32 -- every value rounded where it is stored / widened where it is read.  The results of
        * box2d_iou(precise=True) on fp32 boxes (reference box/__init__.py:204-205, 224: boxes.double(), ious.to(dtype)) without
        * the fp64 copy of the matrix: a third of the bytes. */
       D3D_F64_M32 = 2,
       /* d3d_iou2d_forward / _backward (BOX / RBOX), d3d_nms2d: everything in memory f32 (boxes, scores, the matrix), the arithmetic f64 --
        * every value widened where it is loaded.  box2d_iou / box2d_nms (precise=True) on fp32 tensors without the .double()
        * copies either (box/__init__.py:204-205, 254-255). */
       D3D_F32_WIDE = 3,
       /* d3d_table_conv / d3d_table_conv_wgrad only: IEEE half and bfloat16 in memory, fp32 accumulation on the matrix cores */
       D3D_F16 = 4, D3D_BF16 = 5 };

/* status bits OR-ed into counts[D3D_COUNT_STATUS] by the voxel kernels */
enum { D3D_VOXEL_STATUS_COORD_OVERFLOW = 1,   /* sparse: 2^20 <= |floor(p/size)| < 2^31 (NaN, inf and
                                                 larger values become the reference's INT_MIN coordinate) */
       D3D_VOXEL_STATUS_TABLE_FULL = 2,       /* internal hash table overflow (cannot happen
                                                 with the documented workspace size)           */
       D3D_VOXEL_STATUS_PACK_OVERFLOW = 4,    /* a voxel holds more points than the packed one-word
                                                 hash slot can count: results are invalid; repeat the
                                                 call with D3D_VOXEL_PLAIN_SLOTS                 */
       D3D_VOXEL_STATUS_BIN_OVERFLOW = 8 };   /* binned index: a bucket of the partition holds more distinct
                                                 cells than its LDS table (or > 2 M points): results are
                                                 invalid; repeat the call with D3D_VOXEL_PATH_HASH */
enum { D3D_COUNT_VOXELS = 0, D3D_COUNT_POINTS = 1, D3D_COUNT_STATUS = 2, D3D_COUNT_AUX = 3, D3D_NUM_COUNTS = 4 };

int         d3d_abi_version(void);
int         d3d_last_hip_error(void);           /* hipError_t of the last D3D_ERR_HIP */
const char *d3d_status_string(int status);

/* ------------------------------------------------------------------ d3d/voxel */

/* Per-call options of the voxel entry points that build an index (`flags`, last argument; 0 = automatic).  They are
 * arguments, not library state: two threads / streams may use different ones at the same time, and the retry a caller
 * issues after a PACK_ / BIN_OVERFLOW status touches nothing shared.
 *   D3D_VOXEL_PATH_HASH    hash table in HBM (any input) instead of the default binned index (points partitioned into
 *                          buckets, per-bucket index in LDS; up to 16 M points, grids below 2^32 - 1 cells).  Both give
 *                          identical outputs; see DESIGN.md section 4.
 *   D3D_VOXEL_PLAIN_SLOTS  (hash table) general two-word slots, any count / key width, instead of the default one-word
 *                          slots {count | key | first index} that are used whenever they fit 64 bits.
 *   D3D_VOXEL_SPLIT_FILL   (dense contract, binned index, C == 4) the ranked rows staged by the index, then per-voxel outputs
 *                          and voxels[V,P,C] from two launches (k_meta_first + k_fill_c4) instead of the fused k_emit, which
 *                          reads first rows straight from `points`.  Identical outputs.
 *   D3D_VOXEL_PARTITION_3PASS  (binned index) the partition of rounds 1-3 -- tile histograms, a scan over the tile x bucket
 *                          matrix, one scattered store per point: three launches -- instead of the one-launch tile sort
 *                          (round 4: every tile of 8192 points is sorted by bucket in LDS and written as one coalesced
 *                          run; the bucket workgroups gather their runs).  Identical outputs; frames above 4 M points
 *                          always take the three-pass partition.
 *   D3D_VOXEL_EXACT_MEAN   (dense contract, reduction MEAN) the aggregates of voxels with MORE than max_points points are summed
 *                          sequentially in fp32 in point order, bit for bit like voxelize.cpp:142,164 -- a post-pass (table of
 *                          those voxels, their points compacted in point order, a stable sort by voxel, one wavefront per
 *                          voxel adding in order; ~2x the call).  Default: those voxels are summed in fp64 in arrival order,
 *                          which differs from the reference by ITS rounding error (count * 2^-24 relative) only; voxels within
 *                          max_points, MAX and MIN are bit-exact either way. */
/*   D3D_VOXEL_WIDE_KEYS   (sparse contract) ANY int32 voxel coordinate: the hash table compares all 96 bits of (x, y, z) instead of
 *                          the default 3 x 21-bit key (finite coordinates in (-2^20, 2^20) per axis; beyond it the call comes back
 *                          with D3D_VOXEL_STATUS_COORD_OVERFLOW and is to be repeated with this flag).  Every input
 *                          voxelize.cpp:309 accepts then gives the reference's voxels.  A general path, slower than the default. */
enum { D3D_VOXEL_PATH_HASH = 1, D3D_VOXEL_PARTITION_3PASS = 2, D3D_VOXEL_PLAIN_SLOTS = 4, D3D_VOXEL_SPLIT_FILL = 8,
       D3D_VOXEL_EXACT_MEAN = 16, /* 32: retired */ D3D_VOXEL_WIDE_KEYS = 64, D3D_VOXEL_FLAGS_ALL = 95 };

/* scratch for any of the three voxel entry points on n points / nvox voxels */
size_t d3d_voxelize_workspace_bytes(int64_t n_points, int64_t n_voxels);

/* replaces voxelize_3d_dense (reference d3d/voxel/voxelize.h:9-12, voxelize.cpp:45-199).
 *   points[n,c] f32; shape[3] i32 (host); bound[6] f32 (host: xmin,xmax,ymin,ymax,zmin,zmax)
 *   outputs sized for cap = min(n, max_voxels) voxels:
 *   voxels[cap,max_points,c] f32, coords[cap,3] i64, pmask[cap,max_points] u8 (0/1),
 *   npoints[cap] i32, aggregates[cap,c] f32 (NULL iff reduction == NONE).
 *   Rows >= counts[D3D_COUNT_VOXELS] are not part of the result (the caller slices them off, cf. voxelize.cpp:167-179):
 *   coords / pmask / npoints / aggregates leave them untouched; `voxels` may hold ZEROS there, anywhere inside its cap rows
 *   (round 6: part of the tensor's zero padding is stored under the index launches, over a range fixed before the voxel
 *   count exists -- the buffers MUST have the cap rows stated above, not just the rows a caller expects to come back).
 *   counts: device int64[D3D_NUM_COUNTS]. */
int d3d_voxelize_3d_dense(const float *points, int64_t n, int32_t c,
                          const int32_t *shape, const float *bound,
                          int32_t max_points, int32_t max_voxels, int32_t reduction,
                          float *voxels, int64_t *coords, uint8_t *pmask, int32_t *npoints,
                          float *aggregates, int64_t *counts,
                          void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);

/* d3d_voxelize_3d_dense that also publishes counts[] to the host as soon as they are final, i.e. BEFORE the
 * HBM-bound fill of voxels[V,P,C] is launched: host_counts[0 .. D3D_NUM_COUNTS) = counts, then
 * host_counts[D3D_NUM_COUNTS] = 1 (system-scope release).  host_counts = D3D_NUM_COUNTS + 1 int64 of host-mapped,
 * coherent pinned memory (hipHostMalloc / torch pin_memory) with the flag word cleared by the caller, who polls it:
 * the output sizes (the reference returns exactly-sized tensors, voxelize.cpp:166-180) reach the host while the GPU
 * is still writing the outputs, and the next call can be queued behind them without draining the stream.
 * Exactly ONE notification per call.  Where the binned index with its one-launch partition takes the frame and the output is
 * one launch, the sizes leave from the launch BEFORE the output launch (the bucket index has added up the voxels by then);
 * elsewhere from the first workgroup of the output launch. */
int d3d_voxelize_3d_dense_notify(const float *points, int64_t n, int32_t c,
                          const int32_t *shape, const float *bound,
                          int32_t max_points, int32_t max_voxels, int32_t reduction,
                          float *voxels, int64_t *coords, uint8_t *pmask, int32_t *npoints,
                          float *aggregates, int64_t *counts,
                          void *workspace, size_t workspace_bytes, void *stream, int64_t *host_counts, uint32_t flags);

/* The dense contract into a RESIDENT output buffer (beyond the reference, which returns fresh tensors per frame,
 * voxelize.cpp:166-180; for callers that consume voxels[V,P,C] on the device before the next frame arrives).
 *   voxels[capacity, max_points, c] f32 and row_state[capacity] u16: caller-owned, kept from frame to frame, zero-filled by
 *   the caller ONCE and never written by it; capacity >= min(n, max_voxels) of every call; the same max_points and c in every call.
 * Invariant kept by the call: row r of voxels[v] is zero for r >= row_state[v].  After the call voxels[0 .. V) hold exactly
 * what d3d_voxelize_3d_dense writes (bit for bit, padding included) -- but only the rows that hold points, and zeros over the
 * rows the previous occupant of the same voxel id held, are stored: the zero padding (95 % of the tensor on a LiDAR frame:
 * 1.6 points per voxel at max_points 32) is already there.  The result aliases the buffer: it is valid until the next call
 * on it.  coords / pmask / npoints / aggregates / counts / host_counts (may be NULL) as in d3d_voxelize_3d_dense_notify.
 * D3D_ERR_UNSUPPORTED, with nothing touched: rows of more than 8 floats, buffers not 16-byte aligned, max_points > 256 (c != 4:
 * also max_points * c not a multiple of 4), a frame the binned index does not take (D3D_VOXEL_PATH_HASH, more than 8 M points),
 * D3D_VOXEL_SPLIT_FILL. */
int d3d_voxelize_3d_dense_resident(const float *points, int64_t n, int32_t c,
                          const int32_t *shape, const float *bound,
                          int32_t max_points, int32_t max_voxels, int32_t reduction,
                          float *voxels, uint16_t *row_state, int64_t *coords, uint8_t *pmask, int32_t *npoints,
                          float *aggregates, int64_t *counts,
                          void *workspace, size_t workspace_bytes, void *stream, int64_t *host_counts, uint32_t flags);

/* d3d_voxelize_3d_dense_resident for a caller that keeps the buffer on its user's behalf and hands `voxels` out only while
 * nobody else can see the buffer (VoxelGenerator's pooled default output): the same arguments, launches and results.  The only
 * difference is the label of the output launch in d3d_profile_report: k_emit, the dense call's own, instead of k_emit_resident. */
int d3d_voxelize_3d_dense_pooled(const float *points, int64_t n, int32_t c,
                          const int32_t *shape, const float *bound,
                          int32_t max_points, int32_t max_voxels, int32_t reduction,
                          float *voxels, uint16_t *row_state, int64_t *coords, uint8_t *pmask, int32_t *npoints,
                          float *aggregates, int64_t *counts,
                          void *workspace, size_t workspace_bytes, void *stream, int64_t *host_counts, uint32_t flags);

/* d3d_voxelize_3d_dense_notify split for a caller that pipelines a stream of frames (the reference is a per-frame loop,
 * voxelize.cpp:94; its callers feed it frame after frame): stage 1 = the index launches, stage 2 = the output launch, stage 0 =
 * both.  The two stages may go to two streams (event between them), so that frame k + 1's index -- latency-bound, a few tens of
 * MB -- runs under frame k's output -- bandwidth-bound.  Same arguments in both calls; the workspace carries the index (one
 * workspace per frame in flight).  host_counts may be NULL.  D3D_ERR_UNSUPPORTED for stage != 0 where the output is not one
 * launch (C != 4, unaligned buffers, max_points not a multiple of 16 or above 256, a frame the binned index does not take). */
int d3d_voxelize_3d_dense_staged(const float *points, int64_t n, int32_t c,
                          const int32_t *shape, const float *bound,
                          int32_t max_points, int32_t max_voxels, int32_t reduction,
                          float *voxels, int64_t *coords, uint8_t *pmask, int32_t *npoints,
                          float *aggregates, int64_t *counts,
                          void *workspace, size_t workspace_bytes, void *stream, int64_t *host_counts, uint32_t flags,
                          int32_t stage);

/* replaces voxelize_sparse, bound in Python as voxelize_3d_sparse
 * (reference voxelize.h:14-17, voxelize.cpp:288-335, impl.cpp:5).
 *   points[n,c] f32 (c >= 3); voxel_size[3] f32 (host)
 *   points_mapping[n] i64, coords[n,3] i64 (first counts[0] rows valid), npoints[n] i32. */
int d3d_voxelize_3d_sparse(const float *points, int64_t n, int32_t c, const float *voxel_size,
                           int64_t *points_mapping, int64_t *coords, int32_t *npoints,
                           int64_t *counts, void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);

/* replaces voxelize_filter, bound as voxelize_3d_filter
 * (reference voxelize.h:19-25, voxelize.cpp:337-484).
 *   feats[n,c] f32, points_mapping[n] i64, coords[nvox,3] i64, voxel_npoints[nvox] i32,
 *   coords_bound[6] i64 (host: row-major [3][2] = lo,hi per axis)
 *   out_feats[n,c], out_mask[n] i64, out_mapping[n] i64, out_npoints[nvox] i32,
 *   out_coords[nvox,3] i64;  counts[D3D_COUNT_POINTS] kept points, counts[D3D_COUNT_VOXELS]
 *   kept voxels.  max_points_filter == FARTHEST_SAMPLING -> D3D_ERR_UNSUPPORTED
 *   (reference throws at voxelize.cpp:469-471). */
int d3d_voxelize_3d_filter(const float *feats, int64_t n, int32_t c,
                           const int64_t *points_mapping, const int64_t *coords,
                           const int32_t *voxel_npoints, int64_t nvox, const int64_t *coords_bound,
                           int32_t min_points, int32_t max_points, int32_t max_voxels,
                           int32_t max_points_filter, int32_t max_voxels_filter,
                           float *out_feats, int64_t *out_mask, int64_t *out_mapping,
                           int32_t *out_npoints, int64_t *out_coords,
                           int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* d3d_voxelize_3d_filter directly behind d3d_voxelize_3d_sparse on the same stream, without reading the voxel count
 * back in between (VoxelGenerator.__call__, voxel/__init__.py:93-102, does exactly this pair): coords / voxel_npoints
 * are the sparse call's buffers with nvox_rows rows, sparse_counts its device `counts`; rows >= counts[0] are ignored.
 * max_voxels_filter = DESCENDING is unsupported here (the sort needs the size on the host). */
int d3d_voxelize_3d_filter_chained(const float *feats, int64_t n, int32_t c, const int64_t *points_mapping,
                                   const int64_t *coords, const int32_t *voxel_npoints, int64_t nvox_rows,
                                   const int64_t *sparse_counts, const int64_t *coords_bound,
                                   int32_t min_points, int32_t max_points, int32_t max_voxels,
                                   int32_t max_points_filter, int32_t max_voxels_filter,
                                   float *out_feats, int64_t *out_mask, int64_t *out_mapping,
                                   int32_t *out_npoints, int64_t *out_coords,
                                   int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* VoxelGenerator.__call__'s sparse branch (reference voxel/__init__.py:93-102) in one call: d3d_voxelize_3d_sparse
 * followed by d3d_voxelize_3d_filter on its outputs (same arguments, same outputs as the two calls; the voxel count
 * stays on the device.  max_voxels_filter DESCENDING, round 4: fused as well wherever the binned index runs -- a stable sort
 * of the passing voxels' counts on the device decides the ranks, the output sizes reach host_counts from the LAST launch;
 * D3D_ERR_UNSUPPORTED for it elsewhere: issue the two calls).  Besides saving the round trip it
 * lets the TRIM point filter reuse the per-voxel index ranking the sparse index already holds (voxelize.cpp:457-463)
 * and the voxel filter run inside the index (up to 16 M points, filters NONE / TRIM): points_mapping, coords and npoints
 * are then scratch (not materialised), sparse_counts holds the status bits.
 * Non-finite points get the reference's INT_MIN coordinate on that axis (x86 (int)floor(NaN), voxelize.cpp:309) and are
 * then removed by the coordinate-bound filter exactly as there (:376-384).  Finite points outside the 3 x 21-bit key range
 * (2^20 <= |floor(p/size)| < 2^31) are DROPPED here as long as coords_bound lies inside [-2^20, 2^20] -- the same filter
 * would remove their far-away voxel; d3d_voxelize_3d_sparse alone raises D3D_VOXEL_STATUS_COORD_OVERFLOW for them.
 * Workspace: d3d_voxelize_workspace_bytes(n, n).  host_counts: NULL, or 2 * D3D_NUM_COUNTS + 1 int64 of host-mapped
 * pinned memory with word [D3D_NUM_COUNTS] cleared: receives sparse_counts in [0, 4), counts in [5, 9) and then the flag
 * [4] = 1 before the last kernel (the compaction of the kept points) is launched -- see d3d_voxelize_3d_dense_notify.
 * coord_offset: NULL, or 3 host values subtracted from every row of out_coords -- the `ret.coords - self._offset` that ends
 * VoxelGenerator.__call__ (voxel/__init__.py:103), done where the rows are written instead of by one more launch. */
int d3d_voxelize_3d_sparse_filter(const float *points, int64_t n, int32_t c, const float *voxel_size,
                                  const int64_t *coords_bound, int32_t min_points, int32_t max_points,
                                  int32_t max_voxels, int32_t max_points_filter, int32_t max_voxels_filter,
                                  int64_t *points_mapping, int64_t *coords, int32_t *npoints, int64_t *sparse_counts,
                                  float *out_feats, int64_t *out_mask, int64_t *out_mapping, int32_t *out_npoints,
                                  int64_t *out_coords, int64_t *counts, void *workspace, size_t workspace_bytes,
                                  void *stream, int64_t *host_counts, uint32_t flags, const int64_t *coord_offset);

/* The same call through ONE prepared argument block (round 6): a caller that voxelizes frame after frame fills the block once
 * per generator (sizes, bounds, filters -- what VoxelGenerator.__init__ derives, voxel/__init__.py:16-77) and per frame sets
 * `points`, `n` and `outputs`.  Binding the 26-argument form costs a ctypes / cgo caller more host time per call than the three
 * launches it makes; the intermediates (points_mapping, coords, npoints, both count rows) live at the front of the workspace
 * instead of in caller tensors, the five outputs are carved from ONE caller allocation:
 *   d3d_voxelize_3d_sparse_filter_call_layout(n, c, offsets) -> bytes of `outputs`; offsets[0..4] = byte offsets of
 *     points f32[n,c], points_mask i64[n], points_mapping i64[n], voxel_npoints i32[n], coords i64[n,3] (rows [0, kept) valid);
 *   d3d_voxelize_3d_sparse_filter_call_workspace_bytes(n) -> workspace bytes (the device count rows: its first
 *     2 * D3D_NUM_COUNTS int64 -- sparse_counts, then counts);
 *   d3d_voxelize_3d_sparse_filter_call(call) = d3d_voxelize_3d_sparse_filter on those buffers, same status codes. */
typedef struct D3DSparseFilterCall {
    const float *points;
    int64_t n;
    int32_t c, min_points, max_points, max_voxels, max_points_filter, max_voxels_filter;
    float voxel_size[3];
    uint32_t flags;
    int64_t coords_bound[6];
    int64_t coord_offset[3];
    int32_t has_coord_offset, reserved;
    void *outputs;
    size_t outputs_bytes;
    void *workspace;
    size_t workspace_bytes;
    void *stream;
    int64_t *host_counts;
} D3DSparseFilterCall;
size_t d3d_voxelize_3d_sparse_filter_call_layout(int64_t n, int32_t c, size_t *offsets5);
size_t d3d_voxelize_3d_sparse_filter_call_workspace_bytes(int64_t n);
int d3d_voxelize_3d_sparse_filter_call(const D3DSparseFilterCall *call);

/* ---- beyond the reference: the point-sharded voxelizer of north_star (d3d has no distributed code) ---- */

/* Voxel feature grid without the dense [V,P,C] copy ("dynamic voxelization"): grid semantics of
 * d3d_voxelize_3d_dense (voxelize.cpp:100-101), first-seen voxel ids (voxelize.cpp:119), reduction over
 * ALL in-range points (voxelize.cpp:137-164).  reduction: MEAN/MAX/MIN or 4 = SUM (MEAN without the division).
 *   coords[n,3] i64 (may be NULL when keys is given), npoints[n] i32, aggregates[n,c] f32, first[n] i64 (index_offset + index of the voxel's first
 *   point; may be NULL), mapping[n] i64 (voxel id per point, -1 = out of range; may be NULL),
 *   keys[n + 1] i64 (linear cell index (x*sy+y)*sz+z per voxel, -1 in the rows >= counts[0]; keys[n] = -1 - status
 *   bits of counts[2], so that the status travels with the key list; may be NULL).
 *   Optionally (C == 4, 16-byte aligned points / aggregates / rows) the ranked rows themselves: rows[d3d_voxelize_reduce_rows(n), 4]
 *   f32 receives, per voxel, its first min(count, max_points) points in point order at row seg_base[voxel] (seg_base[n] u32);
 *   max_points = 0 and seg_base = rows = NULL otherwise.  The sharded dense contract sends them to the voxel's owner. */
size_t d3d_voxelize_reduce_rows(int64_t n);
int d3d_voxelize_3d_reduce(const float *points, int64_t n, int32_t c, const int32_t *shape, const float *bound,
                           int32_t reduction, int64_t index_offset, int64_t *coords, int32_t *npoints,
                           float *aggregates, int64_t *first, int64_t *mapping, int64_t *keys,
                           int32_t max_points, uint32_t *seg_base, float *rows, int64_t *counts,
                           void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);

/* Rank-independent compact numbering of occupied cells: mark keys[m] (linear cell index in [0,ncells)) in a
 * bitmap, popcount-prefix it; counts[0] = distinct occupied cells.  lookup: slot[j] = index of keys[j] among the
 * occupied cells in ascending key order (`missing` when unmarked).  Both use the same workspace. */
size_t d3d_grid_compact_workspace_bytes(int64_t ncells);
int d3d_grid_compact_index(const int64_t *keys, int64_t m, int64_t ncells, int64_t *counts,
                           void *workspace, size_t workspace_bytes, void *stream);
int d3d_grid_compact_lookup(const int64_t *keys, int64_t m, int64_t ncells, const void *workspace,
                            size_t workspace_bytes, int64_t missing, int64_t *slot, void *stream);

/* The same index from all-gathered occupancy BITMAPS instead of key lists (for grids whose bitmap, ncells / 8 bytes, is
 * smaller than the key lists: an OR pass replaces one atomic per gathered key): bitmap_mark = this rank's bitmap
 * (ceil(ncells/64) words); compact_from_bitmaps = OR of `world` bitmaps (rank r at parts + r * stride_words) + prefix,
 * counts[0] = distinct cells; compact_keys = the cell of every slot, ascending (key_of_slot[counts[0]]).
 * With owner_ws (d3d_grid_owner_workspace_bytes; world <= 16) compact_from_bitmaps also records, for `rank`, which
 * cells a lower rank has and how many cells every rank OWNS (a cell belongs to the lowest rank that has it -- the rank
 * holding the voxel's first point, shards being contiguous point ranges in rank order). */
int d3d_grid_bitmap_mark(const int64_t *keys, int64_t m, int64_t ncells, unsigned long long *bitmap, void *stream);
size_t d3d_grid_owner_workspace_bytes(int64_t ncells);
int d3d_grid_compact_from_bitmaps(const unsigned long long *parts, int64_t stride_words, int32_t world, int64_t ncells,
                                  int64_t *counts, void *workspace, size_t workspace_bytes, int32_t rank,
                                  void *owner_ws, size_t owner_ws_bytes, void *stream);
int d3d_grid_compact_keys(int64_t ncells, const void *workspace, size_t workspace_bytes, int64_t *key_of_slot,
                          void *stream);

/* Numbering by ownership (bitmap exchange, nvox < 2^24): the voxels a rank owns, in its local first-seen order, are a
 * contiguous run of the global first-seen order, and the runs follow each other in rank order.  scatter_owned writes the
 * reduction's identity into table[nvox, table_stride] (MEAN: c sums + count + id column; else c extrema + id column,
 * counts in cnt_table), then this rank's partial rows at their slots and, for the voxels it owns, the global voxel id
 * in the LAST column; slot_of_local[n_local].  scan_ws: (ceil(n_local/1024) + 2) * 8 + 1024 bytes.  After the all-reduce of
 * the table (same op as the features) finalize_owned reads the id from that column: no exchange of first indices. */
int d3d_sharded_scatter_owned(const int64_t *keys_local, int64_t n_local, int64_t ncells, const void *compact_ws,
                              size_t compact_ws_bytes, const void *owner_ws, size_t owner_ws_bytes, int32_t rank,
                              int64_t nvox, int32_t c, int32_t reduction, const float *agg, const int32_t *cnt,
                              float *table, int32_t table_stride, int32_t *cnt_table, int64_t *slot_of_local,
                              void *scan_ws, size_t scan_ws_bytes, void *stream);
int d3d_sharded_finalize_owned(int64_t nvox, int32_t c, const int64_t *key_of_slot, const float *table,
                               int32_t table_stride, int32_t mean, const int32_t *cnt_in, const int32_t *shape,
                               int64_t *vid_of_slot, int64_t *coords, int32_t *cnt_out, float *feats, void *stream);

/* Steps of the sharded voxelizer around the two all-reduces (no host synchronisation).
 * scatter: keys_all[m] = all-gathered key lists (negative = padding / status rows), already indexed by
 *   d3d_grid_compact_index into compact_ws; rows [begin, begin + n_local) are this rank's own.  Writes the identity
 *   of the reduction into table[nvox, table_stride] (MEAN: c sums + count, else c extrema with the counts in
 *   cnt_table[nvox]) and first[nvox] (INT64_MAX), then this rank's partial rows at their slots, key_of_slot[nvox]
 *   for every gathered key (skipped when NULL), and slot_of_local[n_local] (-1 beyond the rank's voxels).
 * finalize: voxel id of a slot = rank of first[slot] among all first indices (compact_ws sized for n_total cells is
 *   overwritten); slot-ordered all-reduced table -> voxel-id-ordered coords[nvox,3], cnt_out[nvox], feats[nvox,c],
 *   and vid_of_slot[nvox].
 * map: global voxel id of every local point: gmap[i] = vid_of_slot[slot_of_local[local_map[i]]] (-1 stays -1). */
int d3d_sharded_scatter(const int64_t *keys_all, int64_t m, int64_t begin, int64_t n_local, int64_t ncells,
                        const void *compact_ws, size_t compact_ws_bytes, int64_t nvox, int32_t c, int32_t reduction,
                        const float *agg, const int32_t *cnt, const int64_t *first_local, float *table,
                        int32_t table_stride, int32_t *cnt_table, int64_t *first, int64_t *key_of_slot,
                        int64_t *slot_of_local, void *stream);
int d3d_sharded_finalize(int64_t nvox, int32_t c, const int64_t *first, int64_t n_total, int64_t *counts,
                         void *compact_ws, size_t compact_ws_bytes, const int64_t *key_of_slot, const float *table,
                         int32_t table_stride, int32_t mean, const int32_t *cnt_in, const int32_t *shape,
                         int64_t *vid_of_slot, int64_t *coords, int32_t *cnt_out, float *feats, void *stream);
int d3d_sharded_map(int64_t n, const int64_t *local_map, const int64_t *slot_of_local, int64_t nvox,
                    const int64_t *vid_of_slot, int64_t *gmap, void *stream);

/* ---- point-sharded voxelizer, owner-computes exchange (owner.hip; d3d_amd/voxel/sharded.py drives it) ----
 * Every grid cell has one owner rank (a hash of the cell).  A rank sends the partial record of each of its local voxels to
 * the cell's owner (all-to-all), the owner merges the <= world records of a cell in rank order, numbers its voxels in the
 * frame's first-seen order (voxelize.cpp:119) from a one-bit-per-point bitmap whose SUM all-reduce is the OR of the owners'
 * disjoint bit sets, and finishes 1/world of the frame's voxels.  A record is d3d_owner_record_words(c) int32 words:
 * cell key (2), first global point index (2), count (1), c partial features (float bits), padding to an even count. */
int    d3d_owner_record_words(int32_t c);
size_t d3d_owner_pack_workspace_bytes(int64_t n, int32_t world);
/* outputs of d3d_voxelize_3d_reduce (keys[n + 1], cnt[n], agg[n, c], first[n], its counts) -> send[n, words] grouped by owner
 * rank, perm[n] (send position -> local voxel), pos_of_local[n] (its inverse), send_counts[2 world + 1] (device: records per
 * destination, the shard's status bits, rows per destination).  Dense contract (max_points > 0, c == 4): seg_base / rows_local
 * as left by d3d_voxelize_3d_reduce(max_points, ...) -> send_rows[kept rows, 4] with the same grouping, and a record's last word
 * = offset of its rows inside its (source, destination) batch; otherwise max_points = 0 and the three pointers NULL.
 * points / index_offset: the shard that call voxelized -- on the binned index it leaves, instead of rows, the voxels' ranked
 * point INDICES in `rows` (counts[D3D_COUNT_AUX] = 1) and the rows are gathered here; NULL = rows_local holds rows. */
int d3d_owner_pack(const int64_t *keys, const int32_t *cnt, const float *agg, const int64_t *first, const int64_t *counts,
                   int64_t n, int32_t c, int32_t world, int32_t max_points, const uint32_t *seg_base, const float *rows_local,
                   int32_t *send, int32_t *perm, int32_t *pos_of_local, float *send_rows, int64_t *send_counts,
                   void *workspace, size_t workspace_bytes, void *stream, const float *points, int64_t index_offset);
size_t d3d_owner_merge_workspace_bytes(int64_t n_records, int32_t world);
/* recv[R, words] grouped by source rank (src_off[world + 1], device) -> this owner's voxels in GLOBAL ID ORDER, finished
 * (the lowest source rank of a cell holds its first point; the records of one source follow the shard's first-seen order):
 * first_o / coords / npoints / feats (R rows allocated, counts[D3D_COUNT_VOXELS] valid) and rec_owned[R] = owned voxel of
 * every record, lead_rec[R] = leader record of every owned voxel.  reduction: MEAN (sums in rank order, then
 * voxelize.cpp:164's division), MAX, MIN.
 * flags: 0 = up to 2 M records the cells are grouped in LDS, bucket by bucket (three launches, no global atomics); should a
 * bucket not fit (hashed cells: it does) counts[D3D_COUNT_STATUS] carries D3D_VOXEL_STATUS_BIN_OVERFLOW, nothing else is valid
 * and the call is to be repeated with D3D_OWNER_MERGE_CHAINS = the general path (a global hash table with a record chain per
 * cell; taken by itself above 2 M records).  D3D_OWNER_MERGE_TEST_TINY: test hook, buckets overflow at 4 records. */
enum { D3D_OWNER_MERGE_CHAINS = 1, D3D_OWNER_MERGE_TEST_TINY = 2 };
int d3d_owner_merge(const int32_t *recv, int64_t n_records, const int64_t *src_off, int32_t world, int32_t c, int32_t reduction,
                    const int32_t *shape, int64_t *first_o, int64_t *coords, int32_t *npoints, float *feats,
                    int32_t *rec_owned, int32_t *lead_rec, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream,
                    uint32_t flags, const int64_t *point_off);
/* point_off (device, [world]; may be NULL): when the ranks ran d3d_voxelize_3d_reduce with index_offset 0 -- no rank needs the
 * others' shard sizes before its local pass -- the records carry indices local to their source's shard, and point_off[s] =
 * global index of rank s's first point turns the leader's into the voxel's global first point (first_o).  NULL: global already. */
/* dense contract on the owner (voxelize.cpp:128-134: the first max_points points of a voxel by global index = the ranks'
 * candidate rows in rank order): after d3d_owner_merge, with ITS workspace untouched since and ITS flags; recv_rows[*, 4] grouped by source
 * rank (rows_src_off[world + 1], device); lead_rec / npoints / counts_o from d3d_owner_merge.
 * -> voxels[cap_o, max_points, 4], pmask[cap_o, max_points] of the owned voxels in id order (max_points <= 256, c == 4).
 * row_state: NULL, or the resident form of d3d_voxelize_3d_dense_resident -- voxels[capacity >= cap_o, max_points, 4] and
 * row_state[capacity] kept by the caller from frame to frame (zero-filled once): only the rows that hold points and the rows the
 * previous frame left under the same owned id are stored, the zero padding stays; same values in voxels[0 .. Vo). */
int d3d_owner_dense(const int32_t *recv, int64_t n_records, const float *recv_rows, const int64_t *rows_src_off, int32_t world,
                    int32_t max_points, const int32_t *lead_rec, const int32_t *npoints, const int64_t *counts_o, int64_t cap_o,
                    const void *merge_workspace, size_t merge_workspace_bytes, float *voxels, uint8_t *pmask, void *stream,
                    uint32_t flags, uint16_t *row_state);
/* bitmap[(n_total + 63) / 64 + 1] <- bit f for every owned voxel's first point f; the last word = 1 when counts_o carries
 * BIN_OVERFLOW (d3d_owner_merge), else 0 */
int d3d_owner_mark_first(const int64_t *first_o, const int64_t *counts_o, int64_t cap_o, int64_t n_total, uint64_t *bitmap,
                         void *stream);
size_t d3d_owner_number_workspace_bytes(int64_t n_total);
/* global_bits = SUM all-reduce of all owners' bitmaps (with their last word).  vids[i] = global voxel id of owned voxel i;
 * counts_out[D3D_COUNT_VOXELS] = voxels of the whole frame; counts_out[D3D_COUNT_STATUS] = BIN_OVERFLOW when ANY owner's merge
 * has to be repeated (every rank sees the same word: they repeat together). */
int d3d_owner_number(const uint64_t *global_bits, int64_t n_total, const int64_t *first_o, const int64_t *counts_o, int64_t cap_o,
                     int64_t *vids, int64_t *counts_out, void *workspace, size_t workspace_bytes, void *stream);
/* reply[i] = global voxel id of received record i (returned to the record's source rank by the reverse all-to-all) */
int d3d_owner_reply(int64_t n_records, const int32_t *rec_owned, const int64_t *vids, int64_t *reply, void *stream);
/* back[] (ids returned, in send order), pos_of_local (d3d_owner_pack), local_map[n] (point -> local voxel) -> gmap[n] */
int d3d_owner_map(int64_t n, const int64_t *local_map, const int32_t *pos_of_local, const int64_t *back, int64_t *gmap,
                  void *stream);
/* all owners' finished rows -> the replicated feature grid in voxel-id order.  src_off[world + 1] (device; may be NULL): the rows
 * are the ranks' blocks one after the other, block s = rows [src_off[s], src_off[s + 1]), each in ascending id order (what an
 * all-gather of the owners' results delivers) -- merged with coalesced reads and writes (workspace: (nvox / 1024 + 2) * world * 8
 * bytes); NULL: any order, one scattered row each. */
int d3d_owner_replicate(int64_t nvox, const int64_t *vids, const int64_t *coords_in, const int32_t *cnt_in,
                        const float *feats_in, int32_t c, int64_t *coords, int32_t *cnt, float *feats, void *stream,
                        const int64_t *src_off, int32_t world, void *workspace, size_t workspace_bytes);

/* ---- points in 3D boxes: Target3DArray.crop_points / paint_label (reference d3d/abstraction.pyx:308-324,
 * 654-687), per pair box3dr_contains (d3d/dgal_wrap.h:6-19): closed z interval in fp32, the rotated rectangle's bounding
 * box, the rectangle.  points[n, point_stride >= 3] f32 (x, y, z first); box row i = (x, y, z, lx, ly, lz, rz) at
 * boxes + i * box_stride + box_offset ([M,7]: 7, 0; the [n,9] rows of Target3DArray.to_numpy: 9, 2). */
int d3d_crop_3dr(const float *points, int64_t n, int32_t point_stride, const float *boxes, int64_t m, int32_t box_stride,
                 int32_t box_offset, uint8_t *out /* [m, n] 0/1 */, void *stream);
/* idarr[n] u16 = 1 + the lowest index of a box that contains the point and whose class labels[i] (u8) equals semantics[j]
 * (u8), 0 where there is none -- what the reference's descending paint loop leaves (abstraction.pyx:662-673) -- without the
 * bool[m, n] mask. */
int d3d_paint_label(const float *points, int64_t n, int32_t point_stride, const uint8_t *semantics, const float *boxes,
                    int64_t m, int32_t box_stride, int32_t box_offset, const uint8_t *labels, uint16_t *idarr, void *stream);

/* ---- points to cameras: TransformSet.transform_points / project_points_to_camera (reference d3d/abstraction.pyx:971-977,
 * 979-1035).  points[n, stride >= 3] in `dtype` (D3D_F32 or D3D_F64; x, y, z first), read in place; all arithmetic fp64, no
 * contraction.  One camera record, HOST memory (the entry point copies the records into the kernel arguments):
 *   rt: rows 0..2 of the 4x4 extrinsic frame_from -> frame_to, row-major 3x4;  P: the camera's stored 3x3 intrinsic (the axis
 *   rotation of set_intrinsic_camera(rotate=True) already folded in);  fx, fy, cx, cy: intri_matrix[0,0], [1,1], [0,2], [1,2]
 *   and dist = (k1, k2, p1, p2, k3), read only where has_dist != 0;  width, height: the image size in pixels. */
typedef struct D3DCamera {
    double rt[12];
    double P[9];
    double fx, fy, cx, cy;
    double dist[5];
    int32_t width;
    int32_t height;
    int32_t has_dist;
    int32_t reserved;           /* pads the record to 256 bytes */
} D3DCamera;

enum { D3D_PROJECT_ALL_UV = 1,      /* uv row i = point i (remove_outlier=False); without it uv row j = the j-th point in view */
       D3D_PROJECT_DMASK = 2 };     /* also list the points in front of the camera (return_dmask=True) */

size_t d3d_project_points_workspace_bytes(int64_t n, int32_t ncam);
/* abstraction.pyx:979-1035 for ncam >= 1 cameras over one cloud, which is read once per 8 cameras.  Per point and camera
 *   cam = rt . (x, y, z, 1);  h = P . cam;  d = h[2];  u = h[0] / d;  v = h[1] / d        (:991-996, IEEE divisions)
 *   dmask = d > 0;  mask = 0 < u < width and 0 < v < height and dmask                      (:999-1000)
 * and with has_dist the +-20 px mask on the undistorted (u, v), the distortion and the second mask of :1006-1024.
 * Camera c writes its own section of each output (device memory, upper-bound sized):
 *   uv[ncam, n, 2] f64: rows 0 .. K-1 = (u, v) of the points in view in point order, or with D3D_PROJECT_ALL_UV every point's;
 *   mask[ncam, n] i64: entries 0 .. K-1 = the ascending indices of the points in view (np.where, :1029);
 *   dmask[ncam, n] i64 (D3D_PROJECT_DMASK; else may be NULL): entries 0 .. Kd-1 = those of the points with d > 0 (:1030);
 *   counts[ncam, 2] i64 = (K, Kd), final once the call's second launch has run.
 * Three launches per 8 cameras (count, a scan of the workgroups' counts, emit); no launch waits on another workgroup, nothing
 * synchronises.  n <= 2^31 - 1.  Results per camera do not depend on the other records of the call. */
int d3d_project_points(const void *points, int64_t n, int32_t stride, int32_t dtype, const D3DCamera *cameras /* host */,
                       int32_t ncam, uint32_t flags, double *uv, int64_t *mask, int64_t *dmask, int64_t *counts,
                       void *workspace, size_t workspace_bytes, void *stream);
/* abstraction.pyx:971-977: out[n, stride] f64, columns 0..2 = rt[0:3, 0:3] . p + rt[0:3, 3] (rt: host, row-major 3x4 f64), the
 * other columns widened to f64 as numpy's concatenate promotes them. */
int d3d_transform_points(const void *points, int64_t n, int32_t stride, int32_t dtype, const double *rt /* host */, double *out,
                         void *stream);

/* ------------------------------------------------------------------ d3d/point ("next" row) */

/* replaces aligned_scatter_forward[_cuda] / aligned_scatter_backward[_cuda] (reference d3d/point/scatter.h:39-56,
 * scatter.cpp:81-200, scatter_cuda.cu).  coord[n, dim+1] (batch index first), image[batch, channels, dims[0..dim-1]],
 * out / grad [n, channels], all in `dtype`; dims: host int64[dim]; align_type 1 = MEAN, 2 = LINEAR (others ->
 * D3D_ERR_UNSUPPORTED like the reference's py::value_error).  backward ACCUMULATES into image_grad (atomics).
 * workspace (d3d_aligned_scatter_workspace_bytes; may be NULL): a channels-last copy of the map / of the gradient
 * accumulator, which turns the per-channel requests of a point's neighbours into coalesced ones (channels >= 8). */
size_t d3d_aligned_scatter_workspace_bytes(int64_t batch, int64_t channels, const int64_t *dims, int32_t dim, int32_t dtype);
int d3d_aligned_scatter_forward(const void *coord, int64_t n, int32_t dim, const void *image, int64_t batch,
                                int64_t channels, const int64_t *dims, int32_t align_type, int32_t dtype, void *out,
                                void *workspace, size_t workspace_bytes, void *stream);
int d3d_aligned_scatter_backward(const void *coord, int64_t n, int32_t dim, const void *grad, int64_t batch,
                                 int64_t channels, const int64_t *dims, int32_t align_type, int32_t dtype,
                                 void *image_grad, void *workspace, size_t workspace_bytes, void *stream);

/* opt-in per-kernel timing with HIP events on the launch stream (bench.py's roofline leg);
 * report: "kernel,calls,total_ms" lines. */
int d3d_profile_enable(int on);
int d3d_profile_report(char *buf, size_t buf_bytes);

/* what the calling thread's last d3d_voxelize_3d_dense[_notify] launched (measurement only, bench.py): out4[0] = 1 when the
 * output left through the two-role launch (k_emit_split), out4[1] = voxel ids whose zero padding was stored under the index
 * launches, out4[2] / out4[3] = bytes of zeros the filler workgroups of k_tile_sort / k_first_count stored.  No reference
 * counterpart (voxelize.cpp:56-59 zero-fills with torch::zeros). */
int d3d_voxelize_dense_last_plan(int64_t *out4);

/* stream-bandwidth probe on the caller's buffer (bench.py: "fraction of the measured copy bandwidth of the same box",
 * SURVEY 8d).  mode 0 = nontemporal 16-byte stores over `bytes`, 1 = copy first half -> second half, 2 = read sweep,
 * 3 = hipMemsetAsync (the runtime's fill, for reference), 4 / 5 = nontemporal stores in the launch shapes of the output kernel /
 * of the IoU fill, 6 = an empty launch (the overhead of the event pair that d3d_profile_* puts around every launch). */
int d3d_stream_probe(int mode, void *buf, size_t bytes, void *stream);

/* -------------------------------------------------------------------- d3d/box */

/* replaces iou2d_forward[_cuda] (iou_type BOX), the `ious` output of iou2dr_forward[_cuda] (RBOX), of giou2dr_forward[_cuda]
 * (GRBOX) and of diou2dr_forward[_cuda] (DRBOX)  (reference d3d/box/iou.h:7-69, iou.cpp:12-46,95-141,213-258,322-367,
 * iou_cuda.cu:10-48,100-151,216-440).  boxes1[n,5], boxes2[m,5] = (x,y,w,h,r) in `dtype`;
 * ious[n,m] in `dtype`, row-major.  64-bit pair indexing (cf. iou_cuda.cu:36,137).  The workspace is optional
 * (NULL/0 selects the single-kernel path); with it RBOX runs as zero-fill + candidate list + dense clipping, and GRBOX /
 * DRBOX of more than 65536 pairs as a pair kernel for the boxes that are apart (hull / diameter only) + a list of the pairs
 * that need the clip or the tie rules + one listed pair per lane.  A pair's value is the same on every path.
 * Matrices of up to 65536 pairs (BOX / RBOX) take one launch with one pair per lane, with or without a workspace.
 * GIoU = IoU - (H - U) / H, H = area of the convex hull of the two rectangles, U = union area; DIoU = IoU - d^2 / D^2,
 * d = distance of the centres, D = diameter of that hull (dgal's source is not vendored: the published definitions);
 * a rectangle of non-positive area gives 0 for every type.  GBOX / DBOX are D3D_ERR_UNSUPPORTED (the reference's Python
 * layer raises "Unrecognized iou type!" for them, box/__init__.py:216-217).
 * dtype D3D_F64_M32 (BOX / RBOX; GRBOX / DRBOX: D3D_ERR_UNSUPPORTED): boxes f64, ious f32; above 65536 pairs the workspace is
 * required (D3D_ERR_WORKSPACE without it; size: the query with D3D_F64_M32).
 * The query is the largest of what the forward, the backward and the two-kernel routes of GRBOX / DRBOX carve for n x m boxes
 * (fp64 geometry for every dtype but D3D_F32), with one exception: the GRBOX / DRBOX backward of more than 2^33 pairs wants
 * n x ceil(m / 64) words of marks, which the query does not follow -- it runs its single kernel unless more is passed. */
size_t d3d_iou2d_workspace_bytes(int64_t n, int64_t m, int32_t dtype);
int d3d_iou2d_forward(const void *boxes1, int64_t n, const void *boxes2, int64_t m,
                      int32_t iou_type, int32_t dtype, void *ious,
                      void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);
/* flags of d3d_iou2d_forward: 0, or D3D_IOU_LIST_CAP(k) = use only k entries of the candidate list (tests of the
 * overflow -> single-kernel fallback) */
#define D3D_IOU_LIST_CAP(k) ((uint32_t)(k) << 8)

/* replaces iou2d_backward[_cuda] (BOX), iou2dr_backward[_cuda] (RBOX), giou2dr_backward[_cuda] (GRBOX) and
 * diou2dr_backward[_cuda] (DRBOX)  (reference iou.h:14-69, iou.cpp:48-93,143-211,260-320,369-419): grad[n,m] ->
 * grad_boxes1[n,5], grad_boxes2[m,5] (overwritten), all in `dtype`.  The flags the reference saves in forward (nx,
 * xflags, ...) are not needed: the geometry is recomputed analytically.
 * Workspace: d3d_iou2d_workspace_bytes(n, m, dtype); required for BOX / RBOX, optional for GRBOX / DRBOX (with it, matrices
 * of more than 65536 pairs take a gradient kernel for the pairs that are apart and the complete routine for the rest).
 * dtype D3D_F64_M32 (BOX / RBOX): boxes and grad_boxes f64, grad[n,m] f32 (widened as it is read); D3D_F32_WIDE: boxes f32 too,
 * grad_boxes still f64 (the sums are kept in f64: round them once).  grad_boxes2 == grad_boxes1 + 5 n (one buffer): cleared by
 * one launch. */
int d3d_iou2d_backward(const void *boxes1, int64_t n, const void *boxes2, int64_t m, const void *grad,
                       int32_t iou_type, int32_t dtype, void *grad_boxes1, void *grad_boxes2,
                       void *workspace, size_t workspace_bytes, void *stream);

/* the autograd bookkeeping outputs of iou2dr_forward (nx, xflags: iou.cpp:125-141), giou2dr_forward (nxm = {nx, nm},
 * xmflags = {xflags, mflags}: iou.cpp:243-258) and diou2dr_forward (nxd = {nx, far[0], far[1]}, xflags: iou.cpp:352-367).
 * Any output pointer may be NULL.  Per pair (i, j), row-major:
 *   nx[n,m]        vertex count of the intersection polygon (0 when there is none)
 *   xflags[n,m,8]  origin of its vertices, CCW: 0x00 | c = corner c of box 1 (inside box 2); 0x10 | c = corner c of box 2;
 *                  0x20 | e1 << 2 | e2 = crossing of edge e1 of box 1 (corner e1 -> e1 + 1) with edge e2 of box 2; 0xff unused
 *   nm[n,m], mflags[n,m,8]   vertex count of the convex hull of the two rectangles and the corner (0..3 box 1, 4..7 box 2)
 *                  at every hull vertex, CCW from the lowest (x, y); 0xff unused
 *   far[n,m,2]     the two corners (same numbering, far[0] < far[1]) farthest apart -- the hull's diameter
 * (dgal's own flag encoding is not published; this library's backward ignores the arrays.)  xflags / mflags 8-byte aligned. */
int d3d_iou2dr_flags(const void *boxes1, int64_t n, const void *boxes2, int64_t m, int32_t dtype, uint8_t *nx,
                     uint8_t *xflags, uint8_t *nm, uint8_t *mflags, uint8_t *far, void *stream);

/* replaces pdist2dr_forward[_cuda] / pdist2dr_backward[_cuda] (reference d3d/box/dist.h:7-20, dist.cpp:10-110,
 * dist_cuda.cu:10-80; Python box2dr_pdist / box3dr_pdist, box/__init__.py:333-381): SIGNED distance from points[n,2] to the
 * boundary of boxes[m,5], positive inside; dist[m,n] (box-major, as dist.cpp:39), iedge[m,n] (may be NULL) = nearest edge k
 * (corner k -> k + 1) or 4 + k when the nearest boundary point is corner k.  backward: grad[m,n] -> grad_boxes[m,5],
 * grad_points[n,2] (both overwritten; the reference's CUDA kernel accumulates them with a data race, dist_cuda.cu:78-79).
 * A call that returns D3D_ERR_BAD_ARG has written nothing. */
int d3d_pdist2dr_forward(const void *points, int64_t n, const void *boxes, int64_t m, int32_t dtype, void *dist,
                         uint8_t *iedge, void *stream);
int d3d_pdist2dr_backward(const void *points, int64_t n, const void *boxes, int64_t m, const void *grad, int32_t dtype,
                          void *grad_boxes, void *grad_points, void *stream);

/* batched box3dr_iou (rotated=1) / box3d_iou (rotated=0)
 * (reference d3d/dgal_wrap.h:45-91; pair loop d3d/tracking/matcher.pyx:57-80).
 * boxes[.,7] f32 = (x,y,z,lx,ly,lz,rz); out[n,m] f32. */
size_t d3d_iou3d_workspace_bytes(int64_t n, int64_t m);
int d3d_iou3d_forward(const float *boxes1, int64_t n, const float *boxes2, int64_t m,
                      int32_t rotated, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* extension (the reference has the [n,m] matrices only): the PAIRED forms a regression loss wants -- box i of boxes1 against
 * box i of boxes2, n pairs, one pair per lane in one launch (boxpair.hip).  d3d_iou2d_paired: ious[i] is the DIAGONAL of
 * d3d_iou2d_forward -- entry [i,i] of the matrix of the same boxes, type and arithmetic, bit for bit where the matrix takes
 * its single-launch route; iou_type BOX / RBOX / GRBOX / DRBOX, any other: D3D_ERR_UNSUPPORTED.  d3d_iou3d_paired: the diagonal
 * of d3d_iou3d_forward (rows (x,y,z,lx,ly,lz,rz); rotated = 1: box3dr_iou, 0: box3d_iou), here for f64 as well: BEV IoU times
 * max(min(zmax) - max(zmin), 0) / max(max(zmax) - min(zmin), 1e-6), 0 where the BEV IoU is 0; no clipping of the dimensions.
 *   dtype: D3D_F32, D3D_F64, or D3D_F32_WIDE = boxes and ious f32 in memory, the arithmetic (and jac) f64, every value widened
 *   where it is loaded and rounded once where it is stored; any other: D3D_ERR_UNSUPPORTED.
 *   jac (may be NULL): [n,10] (2-D) / [n,14] (3-D) in the ARITHMETIC's type (f32 for D3D_F32, f64 otherwise), row i = the partial
 *   derivatives of ious[i] by the 5 (7) parameters of boxes1[i], then by those of boxes2[i] -- a pair owns its row, so the
 *   backward pass is grad[i] * jac[i,:] with no atomics.  A box of non-positive area (RBOX / GRBOX / DRBOX), a pair apart (BOX /
 *   RBOX / 3-D), z ranges that do not overlap: value 0 and a row of zeros, never NaN; the 1e-6 floor, where active, does not move.
 *   n == 0: nothing is done; a null boxes1 / boxes2 / ious with n > 0, n < 0: D3D_ERR_BAD_ARG, nothing written.  No workspace,
 *   no allocation, no synchronisation, work on `stream` only, capturable in a graph. */
int d3d_iou2d_paired(const void *boxes1, const void *boxes2, int64_t n, int32_t iou_type, int32_t dtype,
                     void *ious, void *jac, void *stream);
int d3d_iou3d_paired(const void *boxes1, const void *boxes2, int64_t n, int32_t rotated, int32_t dtype,
                     void *ious, void *jac, void *stream);

/* extension: the SPARSE form of the two matrices (boxsparse.hip) -- the entries of d3d_iou2d_forward (cols = 5, rows (x,y,w,h,r))
 * or d3d_iou3d_forward (cols = 7, rows (x,y,z,lx,ly,lz,rz)) that are strictly above `threshold`, as a list ordered by row and
 * then by column, without the matrix: pairs[k] = (i, j), values[k] = entry [i,j] bit for bit, offsets[n + 1] the CSR row starts
 * (offsets[n] = K).  The comparison is made on the stored value against the threshold rounded to the stored type; NaN is never
 * above it.  Two phases, because only the device knows K: _count fills offsets; the caller reads offsets[n], allocates and calls
 * _emit with the same inputs.  Every pair of bounding boxes is tested (no spatial broad phase); only the candidates are clipped,
 * in both phases.
 *   iou_type: D3D_IOU_BOX / D3D_IOU_RBOX, any other: D3D_ERR_UNSUPPORTED (the loss variants are nonzero almost everywhere).
 *   dtype: cols = 5: D3D_F32, D3D_F64, D3D_F32_WIDE (boxes and values f32 in memory, the arithmetic f64, the value rounded to f32
 *   before the comparison); cols = 7: D3D_F32 only, as d3d_iou3d_forward; any other: D3D_ERR_UNSUPPORTED.
 *   D3D_ERR_BAD_ARG, nothing written: n or m negative or above 2^31 - 1, cols not 5 or 7, a threshold that is negative, NaN or
 *   infinite, a null pointer with work to do, _emit with capacity < offsets[n].  n == 0 or m == 0: D3D_OK without a launch, null
 *   pointers allowed (_count clears a non-null offsets).  pairs[capacity,2] / values[capacity] beyond K stay untouched.
 *   Workspace: d3d_iou_sparse_workspace_bytes(n, m) -- the bounding boxes of boxes2 and one sum per 1024 rows: O(n + m); each phase
 *   fills it for itself, nothing has to survive between them but offsets.  _count does not synchronise; _emit waits for `stream`
 *   once to read offsets[n] (after the caller's own read that word is ready: the wait is a round trip, no more). */
size_t d3d_iou_sparse_workspace_bytes(int64_t n, int64_t m);
int d3d_iou_sparse_count(const void *boxes1, int64_t n, const void *boxes2, int64_t m, int32_t cols, int32_t iou_type,
                         int32_t dtype, double threshold, int64_t *offsets, void *workspace, size_t workspace_bytes,
                         void *stream);
int d3d_iou_sparse_emit(const void *boxes1, int64_t n, const void *boxes2, int64_t m, int32_t cols, int32_t iou_type,
                        int32_t dtype, double threshold, const int64_t *offsets, int64_t capacity, int64_t *pairs,
                        void *values, void *workspace, size_t workspace_bytes, void *stream);

/* replaces the pair loops of BaseMatcher.prepare_boxes (reference d3d/tracking/matcher.pyx:46-80) for the metrics IoU
 * (rotated = 0: box3d_iou) and RIoU (rotated = 1: box3dr_iou): src[n,9], dst[m,9] f32 rows = (label, score, x, y, z, lx, ly,
 * lz, yaw) as Target3DArray.to_numpy lays them out (abstraction.pyx:263-272); the dimensions are clipped to +-1e3
 * (matcher.pyx:49-51); cache[n,m] f32 = 1 - iou.  Workspace: d3d_iou3d_workspace_bytes(n, m) (optional). */
int d3d_match_distance(const float *src, int64_t n, const float *dst, int64_t m, int32_t rotated, float *cache,
                       void *workspace, size_t workspace_bytes, void *stream);

/* replaces ScoreMatcher.match + match_by_order (reference d3d/tracking/matcher.pyx:83-162) as the detection evaluator
 * drives them once per score threshold (d3d/benchmarks.pyx:218-238).  dist[n,m] f32 (d3d_match_distance); src_tag[n],
 * dst_tag[m] i32 categories (negative = takes no part); dst_threshold[m] f32 = distance threshold of dst j's category;
 * order[n] i64 = src rows from the best score down.  Every src row, in that order, takes the nearest unassigned dst of its
 * own category with dist <= threshold (ties: lower index).  src_match[n], dst_match[m] i32 = partner or -1.  Because a
 * row's choice depends only on the rows before it, the matching restricted to the first k rows of `order` IS the matching of
 * the score threshold that selects them: one call serves all thresholds.  Any threshold is exact: a row with more than 64
 * dst within its threshold lists its 64 nearest and, if those are all taken when its turn comes, sweeps its whole row for
 * the nearest free one.  status (device i32): bit 0 = some row had more than 64 (informational). */
size_t d3d_score_match_workspace_bytes(int64_t n, int64_t m);
int d3d_score_match(const float *dist, int64_t n, int64_t m, const int32_t *src_tag, const int32_t *dst_tag,
                    const float *dst_threshold, const int64_t *order, int32_t *src_match, int32_t *dst_match,
                    int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* `batches` associations in one call (the evaluator's score thresholds on a frame, benchmarks.pyx:218-238: 40 short chains of
 * launches when issued one by one).  The rows of all problems are stacked: dist[n_total, m], src_tag[n_total], order[n_total],
 * src_match[n_total]; problem b owns rows row_off[b] .. row_off[b + 1] (row_off[batches + 1] i64, device) and its order /
 * src_match / dst_match entries are indices LOCAL to those rows; the destinations (m, dst_tag, dst_threshold) are common,
 * dst_match[batches, m].  Same result per problem as d3d_score_match.
 * Optional indirection (NULL = none): stacked row r takes its distances from dist row row_src[r] and, with mask (u8 [., m], 0 = the
 * pair takes no part), its acceptable pairs from mask row row_mask[r] -- the literal association of matcher.pyx:155-158 (the k-th
 * best source walks the k-th subset row's distances) without materialising a stacked matrix. */
size_t d3d_score_match_batched_workspace_bytes(int64_t n_total, int64_t m, int64_t batches);
int d3d_score_match_batched(const float *dist, const int64_t *row_src, const uint8_t *mask, const int64_t *row_mask,
                            const int64_t *row_off, int64_t batches, int64_t n_total, int64_t m,
                            const int32_t *src_tag, const int32_t *dst_tag, const float *dst_threshold, const int64_t *order,
                            int32_t *src_match, int32_t *dst_match, int32_t *status, void *workspace, size_t workspace_bytes,
                            void *stream);

/* replaces scipy.optimize.linear_sum_assignment as HungarianMatcher.match calls it once per class (reference
 * d3d/tracking/matcher.pyx:188-230): `batches` independent problems in one launch, one workgroup each.  Problem b is the
 * matrix cost[row_idx[r] * ld + col_idx[c]] for r in row_off[b] .. row_off[b + 1], c in col_off[b] .. col_off[b + 1]
 * (row_off, col_off i64[batches + 1], row_idx, col_idx i64, all on the device): gathered by index, no stacked matrix.  cost is
 * D3D_F32 or D3D_F64 (`dtype`); the solver computes in fp64 and reproduces scipy's algorithm step for step (Crouse 2016,
 * scipy's rectangular_lsap), ties included.  row_match[row_off[b] + r] i32 = the column (local to the problem) assigned to
 * row r or -1, col_match[col_off[b] + c] = the row assigned to column c or -1.  max_rows / max_cols bound every problem's
 * sizes (host values: they size the launch).  status (device i32, zeroed here): bit 0 = a NaN or -inf entry, bit 1 = a row
 * without a finite path (scipy raises ValueError for both; the problem's matches stay -1), bit 2 = a problem beyond max_rows /
 * max_cols or the workspace.  Workspace: d3d_lsap_batched_workspace_bytes(batches, sum of rows, sum of columns). */
size_t d3d_lsap_batched_workspace_bytes(int64_t batches, int64_t total_rows, int64_t total_cols);
int d3d_lsap_batched(const void *cost, int32_t dtype, int64_t ld, const int64_t *row_idx, const int64_t *col_idx,
                     const int64_t *row_off, const int64_t *col_off, int64_t batches, int64_t max_rows, int64_t max_cols,
                     int32_t *row_match, int32_t *col_match, int32_t *status, void *workspace, size_t workspace_bytes,
                     void *stream);

/* replaces NearestNeighborMatcher.match + BaseMatcher.match_by_order (reference d3d/tracking/matcher.pyx:164-186, :90-121):
 * the pairs (r, c) of the subsets src_idx[ns], dst_idx[nd] (i64 rows / columns of dist, leading dimension ld) taken from the
 * least distance up; a pair is accepted when neither side is matched yet, src_tag[r] == dst_tag[c] and
 * dist <= dst_threshold[c] (i32 / i32 / f32 per subset position).  src_free[ns] / dst_free[nd] u8 (NULL = all free): 0 = the box
 * was matched by an earlier call and takes no part.  Equal distances: row-major order of (src position, dst position).
 * src_match[ns], dst_match[nd] i32 = the partner's subset position or -1.  Three launches, no synchronisation. */
size_t d3d_nn_match_workspace_bytes(int64_t ns, int64_t nd);
int d3d_nn_match(const float *dist, int64_t ld, const int64_t *src_idx, int64_t ns, const int64_t *dst_idx, int64_t nd,
                 const int32_t *src_tag, const int32_t *dst_tag, const float *dst_threshold, const uint8_t *src_free,
                 const uint8_t *dst_free, int32_t *src_match, int32_t *dst_match, void *workspace, size_t workspace_bytes,
                 void *stream);

/* replaces crop_2dr (reference d3d/box/utils.cpp:9-47, bound at box/impl.cpp as crop_2dr; Python box2dr_crop /
 * box3dp_crop, box/__init__.py:278-315): points[n,2], boxes[m,5] in `dtype`; out[m,n] u8 (0/1),
 * out[i,j] = point j lies in rotated box i (boundary inclusive). */
int d3d_crop_2dr(const void *points, int64_t n, const void *boxes, int64_t m, int32_t dtype, uint8_t *out, void *stream);

/* box3dp_crop for project_axis = 2 in one launch (reference d3d/box/__init__.py:289-315: crop_2dr on gathered columns, then
 * the interval test (p - d / 2 < b) & (b < p + d / 2) as [M,N] tensor operations, :311-313): points[n, point_stride >= 3] f32,
 * boxes[m, box_stride >= 7] f32 rows (x, y, z, lx, ly, lz, rz); out[m,n] u8 (0/1), the same bits as the composition.
 * D3D_ERR_UNSUPPORTED, nothing touched: another axis, m > 4096 or n < 4096 -- compose it from d3d_crop_2dr. */
int d3d_crop_3dp(const float *points, int64_t n, int32_t point_stride, const float *boxes, int64_t m, int32_t box_stride,
                 int32_t project_axis, uint8_t *out, void *stream);

/* stable descending argsort (the role torch::argsort plays inside the reference's nms2d,
 * nms.cpp:103): keys[n] in `dtype` -> order[n] i64; ties keep ascending index.  The order is torch's:
 * by value (-0 == +0), NaN before every number.  Up to 2048 keys: one workgroup in LDS; 2049 .. 131072: a 4-launch
 * sample sort; above: an LSD radix sort. */
size_t d3d_argsort_desc_workspace_bytes(int64_t n, int32_t dtype);
int d3d_argsort_desc(const void *keys, int64_t n, int32_t dtype, int64_t *order,
                     void *workspace, size_t workspace_bytes, void *stream);

/* the larger of the hard-NMS and the soft-NMS layout for n fp64 boxes, each followed by the score order (n i64) and the
 * scratch of d3d_argsort_desc that a call with order == NULL uses */
size_t d3d_nms2d_workspace_bytes(int64_t n);

/* replaces nms2d / nms2d_cuda (reference d3d/box/nms.h:6-18, nms.cpp:10-119,
 * nms_cuda.cu:17-244).  Follows the CPU control flow (nms.cpp:23-59).
 *   boxes[n,5], scores[n] in `dtype`; order[n] i64 = descending argsort of scores (nms.cpp:103), or NULL: the library
 *   sorts the scores itself, as nms2d does (d3d_argsort_desc's order; inside the first kernel for up to 4096 boxes);
 *   suppressed[n] u8 (0/1) output.
 *   HARD: parallel (broad phase + exact IoU + fixed point, see box.hip); sets of up to 4096 boxes (a detector's top-k) take
 *   a five-launch path of their own unless a flag below names a general one.  LINEAR / GAUSSIAN (soft-NMS, nms.cpp:60-94)
 *   are sequential by construction -- every kept box rescales the later boxes it overlaps and the order is re-established
 *   after each -- and run in one workgroup that follows the reference's control flow.
 *   Other IoU types return D3D_ERR_UNSUPPORTED ("Unsupported iou type!", reference common.h:25).
 *   flags (per call, 0 = automatic): D3D_NMS_BROAD_SWEEP = sweep-and-prune broad phase instead of the uniform grid;
 *   D3D_NMS_FORCE_DENSE = the reference's all-pairs bit matrix (nms_cuda.cu layout) instead of candidate lists;
 *   D3D_NMS_SOFT_NO_LDS = soft-NMS state in global scratch; D3D_NMS_CAND_CAP(k) = use only k entries of the candidate
 *   list (tests of the overflow -> dense hand-over); D3D_NMS_GENERAL = the general path (uniform grid) also for sets of up to
 *   4096 boxes; D3D_NMS_TEST_WITHHOLD = test hook: the first workgroup of a one-launch scan (the grid's cell scan; with
 *   D3D_NMS_BROAD_SWEEP the scan of the incoming-list sizes) withholds its total, so the scan gives up after ~0.1 s and hands
 *   the call to the dense path; D3D_NMS_FORCE_LEVELS = the uniform grid's level kernels (roots of the greedy result decided
 *   before any pair is listed; automatic on dense grids: clusters of detections) on any input, implies the general path;
 *   D3D_NMS_ONE_LEVEL = one level of them instead of two (clusters of a few boxes).
 *   All give the same mask.
 *   soft-NMS has no size limit of its own (100 k boxes with most of them alive: seconds).
 *   dtype: D3D_F32 / D3D_F64 (boxes and scores), or D3D_F32_WIDE = f32 in memory, f64 arithmetic (what box2d_nms(precise=True)
 *   computes for fp32 tensors, box/__init__.py:254-255, without the copies). */
enum { D3D_NMS_BROAD_SWEEP = 1, D3D_NMS_FORCE_DENSE = 2, D3D_NMS_SOFT_NO_LDS = 4, D3D_NMS_GENERAL = 8, D3D_NMS_TEST_WITHHOLD = 16,
       D3D_NMS_FORCE_LEVELS = 32, D3D_NMS_ONE_LEVEL = 64,
       D3D_NMS_KEEP_MASK = 128   /* `suppressed` receives the KEEP mask -- what box2d_nms returns, ~suppressed (reference
                                    box/__init__.py:272) -- written by the kernels that decide it instead of a pass over the mask */ };
#define D3D_NMS_CAND_CAP(k) ((uint32_t)(k) << 8)
int d3d_nms2d(const void *boxes, const void *scores, const int64_t *order, int64_t n,
              int32_t iou_type, int32_t suppression_type, int32_t dtype,
              float iou_threshold, float score_threshold, float suppression_param,
              uint8_t *suppressed, void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);

/* d3d_nms2d with a host-mapped word of the CALLER's (hipHostMalloc / pinned, int32, one per thread of callers): hard NMS on
 * the general path learns from it, half-way through ITS OWN launches, whether this call's boxes form clusters (a dense
 * broad-phase grid) -- only then are the ten launches of the level kernels enqueued; a scattered set skips them.  The call
 * waits for that word (the GPU keeps working: the launch that writes it has 18 us of work of its own), so it returns with
 * the second half of its kernels still in flight, like d3d_nms2d.  Same mask either way.  NULL, a stream under capture, or
 * D3D_NMS_FORCE_LEVELS: as d3d_nms2d, which always enqueues the level kernels.  Nothing is remembered between calls. */
int d3d_nms2d_notify(const void *boxes, const void *scores, const int64_t *order, int64_t n,
                     int32_t iou_type, int32_t suppression_type, int32_t dtype,
                     float iou_threshold, float score_threshold, float suppression_param,
                     uint8_t *suppressed, void *workspace, size_t workspace_bytes, void *stream, uint32_t flags,
                     int32_t *host_word);

/* Which route the LAST hard-NMS call that used `workspace` took (waits for `stream`).  Bits of *status:
 *   D3D_NMS_STATUS_DENSE_PATH    the n x n mask + sequential sweep decided the result (candidate list overflowed, a box covered
 *                                more than 1024 grid cells, the fixed point did not settle, D3D_NMS_FORCE_DENSE, or a scan gave up):
 *                                same mask, but seconds instead of microseconds at 100 k boxes;
 *   D3D_NMS_STATUS_SCAN_GAVE_UP  a one-launch scan stopped waiting for an earlier workgroup's total (~0.1 s of polling: a
 *                                preempted queue, a profiler holding workgroups back) and handed over to the dense path -- the
 *                                result is still exact; a caller that sees this on a shared GPU may simply call again.
 * The flags sit in the first bytes of the workspace: ask before anything else uses it.
 * suppression_type != HARD: *status = 0 (soft-NMS has a single route).  The reference has no counterpart (nms.cpp is one loop). */
enum { D3D_NMS_STATUS_DENSE_PATH = 1, D3D_NMS_STATUS_SCAN_GAVE_UP = 2 };
int d3d_nms2d_status(const void *workspace, int32_t suppression_type, void *stream, uint32_t *status);

/* Hard NMS inside every group of a batch -- the (sample, class) groups of a detector's output -- in ONE launch: a workgroup
 * per group, the group's sort, geometry and greedy sweep all in LDS (box.hip, k_nms_group).  The reference has no counterpart:
 * its nms2d is one loop over one set (nms.cpp:10-119), and a caller loops over the groups or shifts their coordinates apart.
 *   boxes[n,5], scores[n] in `dtype` (D3D_F32 / D3D_F64 / D3D_F32_WIDE, as d3d_nms2d); iou_type BOX or RBOX; others return
 *   D3D_ERR_UNSUPPORTED, as does any other dtype.
 *   seg_offsets[ngroups + 1] i64, ascending, seg_offsets[0] >= 0, seg_offsets[ngroups] <= n: group g owns positions
 *   seg_offsets[g] .. seg_offsets[g + 1] - 1 of perm[] (i64 row numbers, each row in at most one group), or of the rows
 *   themselves when perm is NULL (rows already grouped contiguously).  Ties in score keep the order of the positions, so a
 *   STABLE sort of the group ids gives the order d3d_nms2d has on each group alone.
 *   keep[n] u8, indexed by ROW: for every group of at most d3d_nms2d_group_max() boxes (1024: one box per lane of the
 *   largest workgroup) exactly the bytes d3d_nms2d writes for that group's rows alone, given D3D_NMS_KEEP_MASK, the same
 *   thresholds and order = NULL -- key order, the C `float` thresholds against the working type, and the score-threshold tail
 *   that never suppresses the top-ranked box of ITS OWN group (nms.cpp:23-29) included.  A longer group is SKIPPED: its
 *   workgroup returns at once and its keep bytes are not written -- hand it to d3d_nms2d.
 *   max_group: the length of the longest group that is not to be skipped (a host-side hint that only chooses the workgroup
 *   size: up to 256 -> 256 threads and several groups per CU; 0 or less = unknown -> 1024).  A group longer than a hint of
 *   256 or less is skipped like one above the cap.
 *   flags: 0 or D3D_NMS_KEEP_MASK (implied: the keep mask is what is written).  Status code; no allocation, no
 *   synchronisation, work on `stream` only, capturable in a graph.  The workspace is the caller's; the query currently
 *   returns 0 (nothing of a group leaves the LDS) and `workspace` may then be NULL.  n == 0 or ngroups == 0: nothing is done. */
int32_t d3d_nms2d_group_max(void);
size_t d3d_nms2d_grouped_workspace_bytes(int64_t n, int64_t ngroups);
int d3d_nms2d_grouped(const void *boxes, const void *scores, const int64_t *perm, const int64_t *seg_offsets,
                      int64_t n, int64_t ngroups, int32_t max_group, int32_t iou_type, int32_t dtype,
                      float iou_threshold, float score_threshold, uint8_t *keep,
                      void *workspace, size_t workspace_bytes, void *stream, uint32_t flags);

/* ------------------------------------------------------------------ d3d/benchmarks: segmentation */

/* replaces SegmentationEvaluator.collect_labels / collect_labels_pano (reference d3d/benchmarks.pyx:977-1075, called from
 * calc_stats, :1077-1095) for `frames` stacked frames in one call:
 *   gt_labels[n], pred_labels[n] u8; gt_ids[n], pred_ids[n] u16, both NULL for the semantic counts only (collect_labels),
 *   both set for the panoptic ones as well (collect_labels_pano); frame_off[frames + 1] i64 (device), frame f = points
 *   frame_off[f] .. frame_off[f + 1] - 1, frame_off[0] = 0, frame_off[frames] = n, non-decreasing;
 *   class_mask: HOST, 8 words = 256 bits, bit c of word c / 32 set when class c is in `classes`; background 0 .. 255;
 *   outputs [frames, 256], row f = frame f, column = class: tp, fp, fn, itp, ifp, ifn i32 and cumiou f32 -- every entry
 *   written (0 for classes outside the mask; itp .. cumiou are 0 without ids).
 * Counts and match decisions are the reference's, with its "background subtraction" (:1055-1056) read as what it does: it
 * subtracts the 0 that operator[] has just inserted, so a pair's union is g + p - inter always.  cumiou[f][c] is the exact
 * sum of the frame's matched fp32 IoUs rounded once to fp32 (the reference adds them in fp32 in hash-map order), the same
 * bits on every run.  Up to 4 launches (2 without ids), no synchronisation.
 * D3D_ERR_BAD_ARG: frames > 65535, n >= 2^31, only one of the id arrays, a background outside 0 .. 255.
 * Workspace: d3d_segeval_workspace_bytes(n, frames). */
size_t d3d_segeval_workspace_bytes(int64_t n, int64_t frames);
int d3d_segeval(const uint8_t *gt_labels, const uint8_t *pred_labels, const uint16_t *gt_ids, const uint16_t *pred_ids,
                const int64_t *frame_off, int64_t n, int64_t frames, const uint32_t *class_mask,
                int32_t background, int32_t min_points,
                int32_t *tp, int32_t *fp, int32_t *fn, int32_t *itp, int32_t *ifp, int32_t *ifn, float *cumiou,
                void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ d3d/benchmarks: tracking */

/* One frame of TrackingEvaluator.calc_stats (reference d3d/benchmarks.pyx:536-723), every score threshold at once.  All
 * pointers are device memory.  Boxes are [n,9] / [m,9] f32 rows (label, score, x, y, z, lx, ly, lz, yaw); cache[n,m] f32 =
 * d3d_match_distance(dt, gt, rotated = 1).  Classes are slots 0 .. C-1 of the evaluator's classes, -1 = outside them.
 *   dt_cls[n], gt_cls[m] i32 slots; dt_tid[n], gt_tid[m] u64 track ids, unique within the frame;
 *   dt_stid[n] / dt_srow[n], gt_stid[m] / gt_srow[m]: the tids sorted ascending and the row of each;
 *   dt_perm[n] i32: the detections in the reference's score order, np.flip(np.argsort(scores, kind="stable"));
 *   row_off[T + 1] i64: problem t of the association owns rows row_off[t] .. row_off[t + 1], as many as detections are
 *   selected at threshold t (slot class >= 0 and !(score < threshold)); n_total = row_off[T];
 *   capacity: pairs per threshold of the two state buffers, >= m. */
typedef struct D3DTrackFrame {
    const float *dt_boxes;
    const float *cache;
    const int32_t *dt_cls;
    const int32_t *gt_cls;
    const uint64_t *dt_tid;
    const uint64_t *gt_tid;
    const uint64_t *dt_stid;
    const int32_t *dt_srow;
    const uint64_t *gt_stid;
    const int32_t *gt_srow;
    const int32_t *dt_perm;
    const int64_t *row_off;
    int64_t n;
    int64_t m;
    int64_t n_total;
    int64_t capacity;
} D3DTrackFrame;

/* Bytes of one state buffer: count i32[T], then gt_tid u64[T, capacity], dt_tid u64[T, capacity], gt_cls i32[T, capacity],
 * dt_cls i32[T, capacity], each piece starting at a 256-byte boundary.  An all-zero buffer is the empty state. */
size_t d3d_track_state_bytes(int64_t capacity, int32_t thresholds);
size_t d3d_track_workspace_bytes(int64_t n, int64_t m, int32_t thresholds, int64_t n_total);
/* thresholds[T] f32, max_dist[C] f32 (= 1 - min overlap of the class); state_in -> state_out (distinct buffers of
 * d3d_track_state_bytes(capacity, T)); outputs: assign[T, m] i32 = the detection assigned to ground truth j at threshold t
 * (fresh match or kept carry-over) or -1, iou[T, m] f32 = 1 - cache of that pair, counts[T, 3, C] i32 = fp, id switches,
 * fragments.  Three launches (prepare, d3d_score_match_batched, update), no synchronisation.
 * D3D_ERR_BAD_ARG: T outside 1 .. 65535, C outside 1 .. 4096, capacity < m, state_in == state_out, a missing pointer. */
int d3d_track_frame(const D3DTrackFrame *frame, const float *thresholds, int32_t T, const float *max_dist, int32_t C,
                    const void *state_in, void *state_out, int32_t *assign, float *iou, int32_t *counts,
                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ d3d/benchmarks: detection, many frames */

/* DetectionEvaluator.calc_stats's device work (reference d3d/benchmarks.pyx:188-283: BaseMatcher.prepare_boxes,
 * d3d/tracking/matcher.pyx:24-82, and one ScoreMatcher.match per score threshold, matcher.pyx:142-162) for `frames` stacked
 * frames in two launches (deteval.hip).  The reference has no counterpart: it takes one frame per call.  All pointers are device
 * memory.
 *   dt_boxes[N,9], gt_boxes[M,9] f32 rows (label, score, x, y, z, lx, ly, lz, yaw); dt_off[frames + 1], gt_off[frames + 1] i64,
 *   rising from 0 to N / M: frame f owns detections dt_off[f] .. dt_off[f + 1] - 1 (n_f of them) and ground truths gt_off[f] ..
 *   gt_off[f + 1] - 1 (m_f); cache_off[frames + 1] i64, cache_off[0] = 0, cache_off[f + 1] = cache_off[f] + n_f * m_f;
 *   pairs = cache_off[frames]; max_n / max_m: the largest n_f / m_f (the host's statement: the offsets are not read back);
 *   dt_cls[N], gt_cls[M] i32: slots 0 .. C-1 of the evaluator's classes, negative = outside them; max_dist[C] f32;
 *   dt_perm[N] i32: at dt_off[f] the frame's in-class detections (rows local to the frame) from the best score down, the rest
 *   of the stretch unused; dt_rank[N] i32: a detection's position in that order, negative outside the classes;
 *   literal != 0: one problem per (frame, threshold), slots[frames, T] i32 = the detections selected at threshold t (a prefix of
 *   the order); slot k accepts the ground truths of the k-th best selected detection (its class, its own distance <=
 *   max_dist) and takes the free one nearest in the cache row of the k-th selected detection IN INDEX ORDER (matcher.pyx:155-158
 *   as written), ties to the lower index.  Outputs gt_match / gt_iou [T * M]: frame f's block [T, m_f] starts at T * gt_off[f].
 *   literal == 0: one problem per frame, slots[frames] = its in-class detections, every slot walks its own row; gt_match /
 *   gt_iou [M] and dt_match[N] (the ground truth of a detection) in the frames' layout.
 *   gt_match: the matched detection, local to the frame, or -1; gt_iou: 1 - cache of that pair, 0 without one.
 *   cache: the ragged distance cache, frame f's [n_f, m_f] block at cache_off[f], every entry with d3d_match_distance(rotated =
 *   1)'s bits -- or NULL: it lives in the workspace then (d3d_deteval_batched_workspace_bytes(pairs, 0); with a cache given
 *   the workspace is not used and may be NULL).
 * Frames without detections or without ground truths are legal: nothing matches.  d3d_deteval_frame_max(): the largest n_f
 * and m_f the call takes (1024: one wavefront walks a problem, with the frame's state in 4 KB of LDS; a larger frame belongs to
 * d3d_match_distance + d3d_score_match_batched).  Status code; no allocation, no synchronisation, work on `stream` only.
 * D3D_ERR_UNSUPPORTED: max_n or max_m above d3d_deteval_frame_max() -- nothing is launched or written (a frame above the
 * bound in spite of the statement is skipped by its workgroups).  D3D_ERR_BAD_ARG: negative sizes, T outside 1 .. 65535, C outside
 * 1 .. 32767, frames * T >= 2^31, a missing pointer.  D3D_ERR_WORKSPACE: no cache given and the workspace too small. */
int32_t d3d_deteval_frame_max(void);
size_t d3d_deteval_batched_workspace_bytes(int64_t pairs, int32_t cache_given);
int d3d_deteval_batched(const float *dt_boxes, const float *gt_boxes, const int64_t *dt_off, const int64_t *gt_off,
                        const int64_t *cache_off, int64_t frames, int64_t pairs, int64_t max_n, int64_t max_m,
                        const int32_t *dt_cls, const int32_t *gt_cls, const int32_t *dt_perm, const int32_t *dt_rank,
                        const int32_t *slots, int32_t T, const float *max_dist, int32_t C, int32_t literal,
                        float *cache, int32_t *gt_match, float *gt_iou, int32_t *dt_match,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ d3d/math */

/* replaces i0e / i1e / i0e_cuda / i1e_cuda (reference d3d/math/impl.cpp:16-46, math.h:6-11, over the templates of
 * math/bessel.h:16-35, 121-132, 223-238): out[i] = exp(-|x[i]|) I_order(x[i]) for the n elements of a flat fp32 (D3D_F32) or
 * fp64 (D3D_F64) array, order 0 or 1 -- the reference's bits in both dtypes (where it rounds: bessel.hip's header; for fp64
 * these are scipy.special.i0e / i1e's bits).  x and out need the alignment of their element only and may be the same buffer;
 * n is not bounded by 2^31 (the reference's loop index is an int).  One launch, no workspace, no synchronisation; n == 0
 * launches nothing.
 * D3D_ERR_BAD_ARG: order outside {0, 1}, n < 0, a null or misaligned pointer with n > 0; D3D_ERR_UNSUPPORTED: any other dtype
 * (AT_DISPATCH_FLOATING_TYPES in the reference). */
int d3d_bessel_e(int32_t order, const void *x, int64_t n, int32_t dtype, void *out, void *stream);
/* the derivative of i0e, which the reference's I0Exp.backward (d3d/math/__init__.py:19-24) does not compute -- it returns
 * i1e(grad) -- in one pass over x and grad: grad_x[i] = grad[i] * (i1e(x[i]) - sign(x[i]) * i0e(x[i])), sign(0) = 0, both
 * Bessel values with d3d_bessel_e's bits, the multiply, the subtract and the multiply rounded in the dtype, uncontracted.
 * Arguments and errors as d3d_bessel_e; grad_x may be x or grad. */
int d3d_i0e_backward(const void *x, const void *grad, int64_t n, int32_t dtype, void *grad_x, void *stream);

/* ------------------------------------------------------------------ per-voxel pooling of point features (an extension) */

/* Reduces learned per-point rows into their voxels (point -> voxel) and gathers voxel rows back to the points, without float
 * atomics: the mapping is inverted once into a CSR index and every pooling call folds a voxel's rows STRICTLY in ascending point
 * index, so the results are the same bits on every run and for every launch shape.  The reference has no counterpart (its
 * voxelizer reduces the raw input columns only, voxelize.cpp:137-164).
 *
 * d3d_voxel_index: mapping[k] = voxel id in [0, v) of point i, or -1 for "belongs to no voxel" (points_mapping of the sparse
 *   contract).  order[k]: its first K' entries are the mapped points grouped by ascending voxel id, ascending point index inside a
 *   voxel (the rest is scratch); offsets[v + 1]: voxel j owns order[offsets[j] .. offsets[j + 1]), offsets[v] = K';
 *   counts[0] = K', counts[1] = the ids outside [-1, v) -- those points are left out like -1, nothing is accessed out of range.
 *   k and v are at most 2^31 - 1 (D3D_ERR_UNSUPPORTED above).  k == 0: offsets and counts are zeroed.
 * d3d_voxel_pool_forward: feat[k, c] (D3D_F32 / D3D_F64, c >= 1) -> out[v, c].  reduction: D3D_REDUCE_MEAN / MAX / MIN, 4 = SUM
 *   as in d3d_voxelize_3d_reduce.  SUM: 0 + x_0 + x_1 + ... in the dtype, in point order; MEAN: that sum / (T)count, one division;
 *   MAX / MIN: the first point with x > best (x < best) wins, a NaN wins over every number and the first NaN stays, -0.0 == +0.0.
 *   arg (may be NULL; MAX / MIN only, ignored otherwise): [v, c] the winner's point index.  A voxel without points: 0, arg -1.
 *   order / offsets as d3d_voxel_index wrote them (they are trusted).  Rows move as 16-byte vectors when c is a multiple of 4 (f32)
 *   / 2 (f64) and feat, out and arg are 16-byte aligned, element by element otherwise.
 * d3d_voxel_pool_backward: grad_out[v, c] -> grad_feat[k, c], every row written exactly once: row i = grad_out[m] (SUM),
 *   grad_out[m] / (T)(offsets[m + 1] - offsets[m]) (MEAN), grad_out[m, ch] where arg[m, ch] == i and 0 elsewhere (MAX / MIN),
 *   m = mapping[i]; a zero row where m is outside [0, v).  offsets is read for MEAN only, arg for MAX / MIN only.  With SUM this is
 *   the gather "each point gets its voxel's row".
 * D3D_ERR_BAD_ARG: a negative size, c < 1, a missing pointer; D3D_ERR_WORKSPACE: workspace missing or smaller than the query;
 * D3D_ERR_UNSUPPORTED: another reduction or dtype, k or v above 2^31 - 1.  None of them launches anything. */
size_t d3d_voxel_index_workspace_bytes(int64_t k, int64_t v);
int d3d_voxel_index(const int64_t *mapping, int64_t k, int64_t v, int32_t *order, int64_t *offsets, int64_t *counts,
                    void *workspace, size_t workspace_bytes, void *stream);
int d3d_voxel_pool_forward(const void *feat, int64_t k, int32_t c, int32_t dtype, const int32_t *order, const int64_t *offsets,
                           int64_t v, int32_t reduction, void *out, int32_t *arg, void *stream);
int d3d_voxel_pool_backward(const void *grad_out, int64_t v, int32_t c, int32_t dtype, const int64_t *mapping, int64_t k,
                            const int64_t *offsets, int32_t reduction, const int32_t *arg, void *grad_feat, void *stream);

/* ------------------------------------------------------------------ voxel neighbours and the row gather through them (an extension) */

/* What a submanifold sparse convolution needs before its GEMM: for every active voxel the rows of its active neighbours, and the
 * neighbours' feature rows side by side.  No float atomics; the reference has no counterpart.
 *
 * d3d_voxel_neighbors: coords[v, 3] int64 and batch[v] int64 (may be NULL: one batch) -> table[v, K] int32, K = kx * ky * kz, every
 *   k* odd in 1 .. 7, every d* (dilation) >= 1.  Column k = (ix * ky + iy) * kz + iz holds the row of the voxel at
 *   coords[r] + ((ix, iy, iz) - (k* - 1) / 2) * d* with the same batch value, or -1 when there is none: column K - 1 - k is the
 *   opposite offset, the centre column (K - 1) / 2 is r itself, and table[r, k] == u <=> table[u, K - 1 - k] == r.
 *   Any int64 coordinates: the bounds of every axis and of the batch value are measured on the device, one 64-bit mixed-radix key
 *   per voxel is formed over those spans, and a neighbour outside the measured box is absent without a look-up (a shifted key never
 *   aliases another row).  When the product of the four spans exceeds 2^62, counts[2] = 1: the launches that follow the
 *   measurement see it and return at once, table is left untouched.
 *   counts[3]: [0] the entries >= 0 of the table, centres included; [1] the rows whose (batch, coordinate) an earlier-inserted row
 *   already had -- with duplicates the table is unspecified, but every entry stays in [-1, v) and nothing is accessed out of range;
 *   [2] the span overflow flag.  v == 0: counts zeroed, nothing launched.  Launches: bounds, insert (integer atomicCAS into an
 *   open-addressing table of a power-of-two capacity >= 2 v in the caller's workspace), lookup (one lane per entry); the table does
 *   not depend on the insertion order: the same on every run.
 * d3d_neighbor_gather: feat[v, c] (D3D_F32 / D3D_F64, c >= 1) and table[r, k] -> out[r, k, c]: out[i, j, :] = feat[e, :] with
 *   e = table[i, mirrored ? k - 1 - j : j], a zero row where e == -1; every output row is written exactly once.  feat_cols = 1, or
 *   = k for a feat of [v, k, c], of which row [e, j, :] is taken (with `mirrored` this is the gradient of the plain gather before
 *   its sum over j).  table may be any row range of a larger table (table + r0 * k); its entries are trusted to be in [-1, v).
 *   Rows move as 16-byte vectors when c is a multiple of 4 (f32) / 2 (f64) and feat and out are 16-byte aligned, element by element
 *   otherwise.  Offsets are 64-bit: r * k * c may pass 2^31.
 * D3D_ERR_BAD_ARG: a negative size, an even or out-of-range kernel size, a dilation < 1, c < 1, a feat_cols other than 1 or k, a
 *   missing pointer; D3D_ERR_WORKSPACE: workspace missing or smaller than the query; D3D_ERR_UNSUPPORTED: v or r above 2^31 - 1,
 *   k above 343, another dtype.  None of these refusals launches anything.  (A span overflow is not a refusal: the entry returns
 *   D3D_OK, its insert and lookup launches run, find the flag and return at once.) */
size_t d3d_voxel_neighbors_workspace_bytes(int64_t v);
int d3d_voxel_neighbors(const int64_t *coords, const int64_t *batch, int64_t v, int32_t kx, int32_t ky, int32_t kz, int32_t dx, int32_t dy,
                        int32_t dz, int32_t *table, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int d3d_neighbor_gather(const void *feat, int64_t v, int32_t c, int32_t dtype, int32_t feat_cols, const int32_t *table, int64_t r, int32_t k,
                        int32_t mirrored, void *out, void *stream);

/* ------------------------------------------------------------------ the map of a strided sparse convolution (an extension) */

/* From the active input voxels to the active OUTPUT voxels of a convolution with kernel size k, stride s, padding p and dilation d
 * per axis (spconv's SparseConv3d / SparseInverseConv3d), and the two tables that relate their rows.  kernel_size, stride, padding,
 * dilation: three host int32 each (x, y, z); k in 1 .. 7 (even sizes too), s and d in 1 .. 2^24, p in 0 .. 2^24.  K = kx ky kz,
 * column k = (ix ky + iy) kz + iz as in d3d_voxel_neighbors, the offsets uncentred.
 *
 * The map: input i feeds output o through column (ix, iy, iz) when o * s - p + (ix, iy, iz) * d == i on every axis, i.e. when
 *   i + p - (ix, iy, iz) * d is divisible by s (mathematical modulo: negative coordinates floor) and o is the quotient.  An output is
 *   active iff at least one input feeds it; voxels of different batch values never meet.  A pair (v, k) that has an output is a
 *   candidate, numbered v K + k; OUTPUT ROWS ARE NUMBERED IN THE ORDER OF THEIR FIRST CANDIDATE (the reference voxelizer's
 *   first-seen rule): deterministic, a function of the input alone.
 *     table_out[r, k] == v  : output row r reads input row v through column k;   -1: none
 *     table_in[v, k]  == r  : holds exactly when table_out[r, k] == v;           -1: (v, k) is no candidate
 *   so the convolution, its gradient and the inverse convolution are all d3d_neighbor_gather with mirrored = 0 through one of the
 *   two tables (out[r] = sum_k feat[table_out[r,k]] W[k]; grad_feat[v] = sum_k grad_out[table_in[v,k]] W[k]^T).
 * spatial_shape: NULL, or three host int64 (X, Y, Z), each in 1 .. 2^31 - 1.  When given, outputs are kept only for
 *   0 <= o < floor((S + 2 p - d (k - 1) - 1) / s) + 1 (dense conv3d's output size; below 1 on an axis: D3D_ERR_BAD_ARG), and an
 *   input outside [0, S) sets counts[4] = 1.  When NULL every output with a non-empty receptive field is active.
 * Any int64 coordinates: the bounds of the input are measured on the device, the output box is derived from them (and clipped by
 *   spatial_shape), and one 64-bit mixed-radix key per output is formed over the spans of that box and of the batch value.
 *   counts[3] = 1 (span overflow) when those spans multiply to more than 2^62, or when the inputs span 2^62 or more on an axis (the
 *   box arithmetic needs that headroom).  With counts[3] or counts[4] set every later launch of both entries returns at once:
 *   counts[0] = counts[1] = 0 and nothing but counts and the workspace is written.
 *
 * Two entries with ONE host read between them (only the device knows Vout):
 * d3d_sparse_conv_map_count: coords[v, 3] int64, batch[v] int64 (may be NULL) -> counts[5] int64: [0] Vout, [1] the entries >= 0 of
 *   either table (the same number), [2] 0, [3] span overflow, [4] an input outside spatial_shape.  Launches: bounds, frame (one
 *   lane: the box, the verdicts), clear, insert (one lane per (v, k): integer atomicCAS of the output's key into an
 *   open-addressing table, then a 64-bit integer atomicMin of the candidate number on the slot's second word -- the winner is the
 *   first candidate whatever order the lanes arrive in), and the count half of a scan over the marks "first of its slot".
 * d3d_sparse_conv_map_emit: the same inputs and the SAME workspace, untouched since _count; num_out = counts[0] as read by the host
 *   -> out_coords[num_out, 3] int64, out_batch[num_out] int64 (ignored when batch is NULL), table_in[v, K] int32,
 *   table_out[num_out, K] int32, and counts[2] += the failed claims.  Launches: the scan's apply half (the first candidates write
 *   out_coords, out_batch and their row into their slot), then one lane per (v, k), the column fastest: table_in[v, k] = row or -1
 *   (contiguous stores), and the claim of table_out[row, k] (prefilled with -1) by an integer atomicCAS -1 -> v.  A failed claim
 *   means two inputs share (batch, coordinate): (batch, coordinate) must be unique, counts[2] > 0 is how a violation shows (for
 *   inputs that feed at least one output; others are not examined).  Even then, and with a num_out smaller than counts[0] (rows
 *   from num_out on are dropped), every entry of table_in stays in [-1, num_out) and of table_out in [-1, v).  Integer atomics
 *   only; the same bits on every run.  v == 0: counts zeroed / nothing written, nothing launched.
 * Workspace (d3d_sparse_conv_map_workspace_bytes; 0 for arguments the entries refuse): 256 B of bounds, 256 B of frame, 16 B x C
 *   slots with C the smallest power of two >= max(64, 2 v P), and 8 B per 1024 candidates numbers (v K / 1024, rounded up to 256 B):
 *   O(v P), where P = the product over the axes of ceil(k / (s / gcd(s, d))) is the largest number of outputs one input can feed
 *   (v P bounds Vout).  The launches use the smallest power of two >= max(64, 2 min(v P, cells of the output box)) of those slots.
 * D3D_ERR_BAD_ARG: a negative size, a kernel size outside 1 .. 7, s or d < 1, p < 0, a spatial_shape below 1 or without a dense
 *   output, a missing pointer, num_out < 0 or > v P; D3D_ERR_UNSUPPORTED: s, p or d above 2^24, a spatial_shape above 2^31 - 1,
 *   v P above 2^31 - 1; D3D_ERR_WORKSPACE: workspace missing or smaller than the query.  None of these launches anything. */
size_t d3d_sparse_conv_map_workspace_bytes(int64_t v, const int32_t *kernel_size, const int32_t *stride, const int32_t *dilation);
int d3d_sparse_conv_map_count(const int64_t *coords, const int64_t *batch, int64_t v, const int32_t *kernel_size, const int32_t *stride,
                              const int32_t *padding, const int32_t *dilation, const int64_t *spatial_shape, int64_t *counts,
                              void *workspace, size_t workspace_bytes, void *stream);
int d3d_sparse_conv_map_emit(const int64_t *coords, const int64_t *batch, int64_t v, const int32_t *kernel_size, const int32_t *stride,
                             const int32_t *padding, const int32_t *dilation, const int64_t *spatial_shape, int64_t num_out,
                             int64_t *out_coords, int64_t *out_batch, int32_t *table_in, int32_t *table_out, int64_t *counts,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ the table form of a sparse convolution on the matrix cores */

/* out[r] = sum_k feat[table[r, k]] @ W[k] without the gathered [rows, K * C] buffer (csrc/vconv.hip): what subm_conv3d, sparse_conv3d
 * and sparse_inverse_conv3d compute, their forward and both of their matrix gradients, in fp32, fp16 and bf16.
 *
 * d3d_table_conv: feat[src_rows, cin], table[rows, k] int32 (entries in [-1, src_rows), trusted), weight[k, cin, cout], bias[cout] or
 *   NULL -> out[rows, cout] = bias + the sum over kk, in ascending order, of feat[e] @ weight[kk] with
 *   e = table[r, mirrored ? k - 1 - kk : kk] (d3d_neighbor_gather's meaning); entries -1 contribute nothing.  The forward of the three
 *   operators, and their grad_features through the backward table (the mirrored one, or table_in / table_out) with the weight
 *   transposed to [k, cout, cin] by the caller.  One launch, no workspace.  Products accumulate in fp32 on the MFMA units (fp32: the
 *   exact f32 form), the bias is added in fp32 and the sum is rounded once, to nearest even, to the output type.  A row's bits depend
 *   on its own table row, the feat rows it names, the weight and the bias only (finite weights): not on its position, on the other
 *   rows of the launch or on the run.  16-byte loads where feat and weight are 16-byte aligned; offsets are 64-bit.
 * d3d_table_conv_wgrad: grad_weight[kk] = sum_r feat[table[r, col(kk)]]^T (x) grad_out[r] for grad_out[rows, cout] ->
 *   grad_weight[k, cin, cout], the present (row, entry) pairs of a column compacted in row order before they meet the MFMA.  Two
 *   launches: fp32 partial sums per (column, row slab) into the workspace (d3d_table_conv_wgrad_workspace_bytes: slabs x k x cin x
 *   cout floats, the slab count a function of the four sizes), then the slabs added in ascending order and rounded once.  No float
 *   atomics; the order of every sum is fixed by the table and the sizes: the same bits on every run.  rows == 0: grad_weight zeroed.
 * dtype: D3D_F32, D3D_F16 or D3D_BF16 (every array in it).  D3D_ERR_UNSUPPORTED, nothing touched: D3D_F64, cin or cout that is no
 *   multiple of 16 in 16 .. 256, k above 343, rows or src_rows above 2^31 - 1.  D3D_ERR_BAD_ARG: a negative size, k < 1, another
 *   dtype code, a missing pointer; D3D_ERR_WORKSPACE: workspace missing or smaller than the query.  d3d_table_conv with rows == 0
 *   returns D3D_OK before any HIP call. */
int d3d_table_conv(const void *feat, int64_t src_rows, int32_t cin, const int32_t *table, int64_t rows, int32_t k, int32_t mirrored,
                   const void *weight, const void *bias, int32_t cout, int32_t dtype, void *out, void *stream);
size_t d3d_table_conv_wgrad_workspace_bytes(int64_t rows, int32_t k, int32_t cin, int32_t cout);
int d3d_table_conv_wgrad(const void *feat, int64_t src_rows, int32_t cin, const int32_t *table, int64_t rows, int32_t k, int32_t mirrored,
                         const void *grad_out, int32_t cout, int32_t dtype, void *grad_weight, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ------------------------------------------------------------------ pooling through the tables of the sparse convolutions */

/* out[r] = the sum / mean / max / min over the rows table[r, :] names (spconv's SparseMaxPool3d / SparseAvgPool3d) and its gradient
 * (csrc/vtpool.hip), through the tables of d3d_voxel_neighbors and d3d_sparse_conv_map_emit.  One launch each, no workspace, no float
 * atomics; the gathered [rows, k, c] buffer of d3d_neighbor_gather never exists.  The reference has no counterpart.
 *
 * dtype: D3D_F32, D3D_F64, D3D_F16 or D3D_BF16 (feat, out, grad_out and grad_feat in it); c >= 1, k in 1 .. 343; rows, src_rows and
 *   out_rows at most 2^31 - 1.  reduction: D3D_REDUCE_MEAN / MAX / MIN, 4 = SUM as in d3d_voxel_pool_forward.  Offsets are 64-bit:
 *   rows * c may pass 2^31.
 * d3d_table_pool_forward: feat[src_rows, c], table[rows, k] int32 (entries in [-1, src_rows), trusted) -> out[rows, c]: the reduction
 *   over the PRESENT entries of the row only (an absent neighbour is not a zero), column by column in ascending kk, by
 *   d3d_voxel_pool_forward's rules.  SUM: 0 + x_0 + x_1 + ...; MEAN: that sum / (T)n, one IEEE division, n the present entries;
 *   MAX / MIN: the first x > best (x < best) wins, a NaN wins over every number and the first NaN stays, -0.0 == +0.0.  D3D_F16 /
 *   D3D_BF16: SUM and MEAN accumulate and divide in fp32 and round once, to nearest even, to the output type; MAX / MIN are exact
 *   in every type.  arg (may be NULL; MAX / MIN only, ignored otherwise): [rows, c] int16, the winning column kk (int16: k goes to
 *   343, a byte would wrap at kernel size 7).  count (may be NULL): [rows] int32, the present entries of the row.  A row without
 *   present entries: out 0, arg -1, count 0.
 * d3d_table_pool_backward: grad_out[out_rows, c], back_table[rows, k] int32 (entries in [-1, out_rows), trusted) ->
 *   grad_feat[rows, c], every row written exactly once.  back_table is the transposed map of the forward's table: table_in for a
 *   forward through table_out and the other way round (mirrored = 0), a d3d_voxel_neighbors table for itself with mirrored = 1.
 *   Entry e = back_table[v, kk] >= 0 reached row v in the forward through column fk = mirrored ? k - 1 - kk : kk and contributes
 *   grad_out[e] (SUM), grad_out[e] / (T)count[e] (MEAN), grad_out[e, ch] where arg[e, ch] == fk and nothing elsewhere (MAX / MIN);
 *   the contributions are added to 0 in ascending kk.  D3D_F16 / D3D_BF16: contributions and sum in fp32, one rounding.  arg and
 *   count: [out_rows, c] and [out_rows] as the forward wrote them; arg is read for MAX / MIN only, count for MEAN only.
 * Rows move as 16-byte vectors when c is a multiple of 4 (f32) / 2 (f64) / 8 (f16, bf16) and feat, out, arg (grad_out, grad_feat,
 *   arg) are 16-byte aligned, element by element otherwise: the same bits on both paths.  A row's bits depend on its table row and
 *   on the rows that names only: not on its position in the launch, and not on the run.
 * D3D_ERR_BAD_ARG: a negative size, c < 1, k < 1, a missing pointer (arg for a MAX / MIN backward and count for a MEAN backward
 *   among them); D3D_ERR_UNSUPPORTED: another dtype or reduction code, k above 343, rows, src_rows or out_rows above 2^31 - 1.
 *   None of them launches anything.  rows == 0 returns D3D_OK before any HIP call. */
int d3d_table_pool_forward(const void *feat, int64_t src_rows, int32_t c, int32_t dtype, const int32_t *table, int64_t rows, int32_t k,
                           int32_t reduction, void *out, int16_t *arg, int32_t *count, void *stream);
int d3d_table_pool_backward(const void *grad_out, int64_t out_rows, int32_t c, int32_t dtype, const int32_t *back_table, int64_t rows,
                            int32_t k, int32_t mirrored, int32_t reduction, const int16_t *arg, const int32_t *count,
                            void *grad_feat, void *stream);

/* ------------------------------------------------------------------ voxel features at arbitrary points: interpolation and splat */

/* From the voxels back to ARBITRARY points: trilinear (or nearest) interpolation of sparse voxel features at fractional positions
 * -- the devoxelize step of SPVCNN / PVCNN, PV-RCNN's keypoint features, the point head of a sparse U-Net -- and its transpose, the
 * splat of point rows onto the voxels (csrc/vnbr.hip: the corner table; csrc/vinterp.hip: the two folds).  No float atomics; the
 * [K, 8, C] buffer of gathered corner rows never exists.  The reference has no counterpart.
 *
 * d3d_voxel_corners: coords[v, 3] int64 and batch[v] int64 (may be NULL: one batch), unique as for d3d_voxel_neighbors;
 *   positions[k, 3] in `dtype` (D3D_F32 / D3D_F64) in VOXEL UNITS, integer n the centre of voxel n; position_batch[k] int64 (given
 *   exactly when batch is) -> table[k, J] int32 and weights[k, J] in `dtype`, J = corners = 8 (trilinear) or 1 (nearest).
 *   The rules, every operation one rounding in `dtype` (the build does not contract):
 *     per axis b = floor(x), f = x - b (f may come out as exactly 1 for a tiny negative x: that is the rule);
 *     corner j = dx * 4 + dy * 2 + dz is the voxel at b + (dx, dy, dz) with the point's batch value (the last axis fastest);
 *     w_j = (wx * wy) * wz with wa = f_a where the corner's bit on axis a is set, else 1 - f_a;
 *     J = 1: the one corner floor(x + 0.5), weight 1;
 *     a position that is not finite, or not in [-2^62, 2^62) on an axis, has no corners;
 *     a corner outside the measured box of the coordinates (and of the batch values) is absent without a look-up;
 *     an absent corner: table -1, weight 0;
 *     normalize != 0: s = 0 + w_j0 + w_j1 + ... over the PRESENT corners in ascending j, every present weight is stored as w_j / s;
 *       all weights stay 0 where no corner is present or s == 0.
 *   counts[3] as d3d_voxel_neighbors': [0] the entries >= 0 of the table, [1] duplicate (batch, coordinate) rows, [2] the span
 *   overflow flag (then table and weights are left untouched).  Launches: bounds, insert (both d3d_voxel_neighbors' own, also with
 *   k == 0), look-up (one lane per (point, corner), the corner fastest); every dependency is a kernel boundary.  v == 0: table -1
 *   and weights 0 by two fills, counts zeroed.  Workspace: d3d_voxel_corners_workspace_bytes(v), d3d_voxel_neighbors' layout.
 * d3d_table_interp_forward: feat[v, c], table[rows, j], weights[rows, j] -> out[rows, c]: row r is 0, then + (w[r, jj] * feat[table[r,
 *   jj]]) per present entry in ascending jj -- a rounding after the product and one after the sum; absent entries are skipped.
 * d3d_table_interp_backward: grad[rows, c], weights[rows * j] -> grad_feat[v, c], the transpose: voxel u is 0, then + (w[e] * grad[e / j])
 *   over e in order[offsets[u] .. offsets[u + 1]) in that order; order / offsets are what d3d_voxel_index returns for the flattened
 *   table [rows * j] taken as the mapping (ascending voxel, ascending entry number inside one; they are trusted).  A voxel without
 *   entries gets a zero row; every row is written exactly once.  This is also the forward of a splat, whose gradient is
 *   d3d_table_interp_forward.
 * dtype of the two folds: D3D_F32, D3D_F64, D3D_F16 or D3D_BF16 (feat, out, grad, grad_feat in it).  weights: fp64 for D3D_F64, fp32
 *   otherwise.  D3D_F16 / D3D_BF16 multiply and add in fp32 and round once, to nearest even, at the store.  c >= 1; j is 1 or 8;
 *   v and rows * j at most 2^31 - 1; offsets are 64-bit: rows * c may pass 2^31.  Rows move as 16-byte vectors when c is a multiple
 *   of 4 (f32) / 2 (f64) / 8 (f16, bf16) and the feature and output pointers are 16-byte aligned, element by element otherwise: the
 *   same bits on both paths.  A row's bits depend on its own entries only, and every run gives the same bits.  One launch each, no
 *   workspace, nothing read back.
 * D3D_ERR_BAD_ARG: a negative size, c < 1, a corner count other than 1 or 8, a missing pointer, batch without position_batch or the
 *   reverse; D3D_ERR_UNSUPPORTED: another dtype, v or k * J (rows * j) above 2^31 - 1; D3D_ERR_WORKSPACE: workspace missing or smaller
 *   than the query.  None of them launches anything.  rows == 0 (forward) and v == 0 (backward) return D3D_OK before any HIP call. */
size_t d3d_voxel_corners_workspace_bytes(int64_t v);
int d3d_voxel_corners(const int64_t *coords, const int64_t *batch, int64_t v, const void *positions, const int64_t *position_batch, int64_t k,
                      int32_t dtype, int32_t corners, int32_t normalize, int32_t *table, void *weights, int64_t *counts, void *workspace,
                      size_t workspace_bytes, void *stream);
int d3d_table_interp_forward(const void *feat, int64_t v, int32_t c, int32_t dtype, const int32_t *table, const void *weights, int64_t rows,
                             int32_t j, void *out, void *stream);
int d3d_table_interp_backward(const void *grad, int64_t rows, int32_t c, int32_t dtype, const int32_t *order, const int64_t *offsets,
                              const void *weights, int32_t j, int64_t v, void *grad_feat, void *stream);

/* ------------------------------------------------------------------ sparse voxel rows <-> a dense channels-first grid (BEV map) */

/* The exit of a sparse backbone (csrc/vdense.hip): voxel rows [v, c] scattered into a dense grid [n, c, A, B, D] -- spconv's .dense();
 * viewed [n, c * A, B, D] it is the BEV map the 2D heads take -- and the reverse, the values of a dense tensor at the active sites.
 * Each is the other's gradient.  No float atomics, no workspace, nothing waits on another workgroup.  The reference has no counterpart.
 *
 * d3d_vdense_map: coords[v, 3] int64 and batch[v] int64 (may be NULL: every row in sample 0); HOST arrays shape[3] (>= 1) and
 *   origin[3] int64 in coordinate-COLUMN order and axes[3] int32, a permutation of 0, 1, 2: dense axis k walks column axes[k], its
 *   size is shape[axes[k]].  With (A, B, D) those three sizes and (a, b, d) = coords[axes[k]] - origin[axes[k]]:
 *     cell[i] int64 = ((batch[i] * A + a) * B + b) * D + d, or -1 for a row that lies outside: a column outside [origin, origin +
 *       shape) -- tested as (uint64) coord - (uint64) origin < (uint64) shape, so any int64 values are legal -- or a batch value
 *       outside [0, batch_size);
 *     index[batch_size * A * B * D] int32 = the row at every cell, -1 for none: filled with -1 first, then every inside row claims
 *       its cell with an integer compare-and-swap -1 -> i;
 *     counts[2] int64 (zeroed first): [0] the outside rows, [1] the rows whose claim failed (an earlier row holds the cell: a
 *       repeated (batch, coordinate)).  With counts[1] != 0 WHICH of the rows holds a cell depends on the run: refuse the map.
 *   Two fills and one launch (one lane per row; v == 0: the fills alone).
 * d3d_vdense_scatter: feat[v, c] in `dtype`, index[n * cells_per_sample] (a map's, trusted: entries in [-1, v)) -> out[n, c,
 *   cells_per_sample]: out[s, ch, p] = feat[index[s, p], ch] bit for bit where index[s, p] >= 0, else `fill` rounded once (to nearest
 *   even) to the dtype.  EVERY element of out is written exactly once by this one launch: no memset before it.
 * d3d_vdense_gather: dense[n, c, cells_per_sample], index -> out[v, c]: out[index[s, p], ch] = dense[s, ch, p] bit for bit for every
 *   index[s, p] >= 0; rows that no cell names are left untouched (a map without outside rows names every row once).
 * d3d_vdense_tile_cells: the cells of ONE sample a workgroup of the two kernels owns (a stretch; the last one of a sample is
 *   partial).  A stretch without a present cell is filled (scatter) or skipped (gather) without staging anything.
 * d3d_vdense_sparse_cells: a stretch with at most this many present cells moves them element by element instead of through the LDS
 *   tile (the threshold between the two paths of the kernels: the tests put stretches on both sides of it).
 * dtype: D3D_F32, D3D_F64, D3D_F16 or D3D_BF16; elements move as integers of their size (NaN payloads, infinities, -0.0 are kept).
 *   Rows move as 16-byte vectors when c is a multiple of 4 (f32) / 2 (f64) / 8 (f16, bf16) and the row pointer is 16-byte aligned;
 *   planes when cells_per_sample is such a multiple and the grid pointer is 16-byte aligned; element by element otherwise: the same
 *   bits on every path and every run.  All offsets are 64-bit: n * c * cells_per_sample may pass 2^31.
 * D3D_ERR_BAD_ARG: a negative size, batch_size < 1, a shape below 1, axes that are no permutation, a missing pointer with work to do;
 *   D3D_ERR_UNSUPPORTED: another dtype, v above 2^31 - 1, n * cells_per_sample of 2^39 and more.  None of them launches anything.
 *   c == 0, n == 0 or cells_per_sample == 0 (gather: v == 0 as well) return D3D_OK before any HIP call. */
int32_t d3d_vdense_tile_cells(void);
int32_t d3d_vdense_sparse_cells(void);
int d3d_vdense_map(const int64_t *coords, const int64_t *batch, int64_t v, const int64_t *shape, const int64_t *origin, const int32_t *axes,
                   int64_t batch_size, int64_t *cell, int32_t *index, int64_t *counts, void *stream);
int d3d_vdense_scatter(const void *feat, int64_t v, int32_t c, int32_t dtype, const int32_t *index, int64_t n, int64_t cells_per_sample,
                       double fill, void *out, void *stream);
int d3d_vdense_gather(const void *dense, int64_t n, int32_t c, int32_t dtype, const int32_t *index, int64_t cells_per_sample, int64_t v,
                      void *out, void *stream);

/* ------------------------------------------------------------------ the point branch: furthest point sampling and ball query */

/* Pick M well-spread rows of a cloud, then group the rows inside a radius of each (csrc/psample.hip): the first two steps of a
 * PointNet++ set abstraction, PV-RCNN's keypoints, 3DSSD, Voxel R-CNN.  Both return indices only; no atomics, no sort, nothing waits
 * on another workgroup, every run gives the same bits.  The reference has no counterpart.
 *
 * Both read columns 0 .. 2 of rows of `row_stride` (point_stride, center_stride) >= 3 ELEMENTS in `dtype` (D3D_F32 / D3D_F64); the
 * base needs the alignment of one element only.  Every operation below is one rounding in the dtype (the build does not contract):
 *     q(i, c) = ((dx * dx) + (dy * dy)) + (dz * dz),  dx = x_i - x_c, dy = y_i - y_c, dz = z_i - z_c.
 *
 * d3d_furthest_point_sample: segment b holds the rows point_offsets[b] .. point_offsets[b + 1] and gets M_b = sample_offsets[b + 1] -
 *   sample_offsets[b] samples at indices[sample_offsets[b] ..] (int64, GLOBAL row numbers) and, where distances is not NULL, at
 *   distances[sample_offsets[b] ..] in `dtype`.  Both offset arrays are DEVICE int64[segments + 1], nondecreasing from 0 (to n, and to
 *   the number of samples), and TRUSTED: the caller has checked them (every segment at most 2^31 - 1 rows; no segment with 0 rows and
 *   M_b > 0 -- such a segment would get indices -1 and NaN distances).  The rule, per segment:
 *     a row is EXCLUDED when one of its three coordinates is not finite; every other row starts with d_i = +inf;
 *     step s = 0 .. M_b - 1: c_s = the non-excluded row with the largest d, the LOWEST such row on a tie; indices[s] = c_s and
 *       distances[s] = d_{c_s} as it is BEFORE the update (distances[0] = +inf, then the non-increasing coverage radius squared);
 *       then, for every non-excluded row i, q = q(i, c_s) and d_i = q if q < d_i;
 *     M_b above the segment's rows is legal: once every d is 0 the lowest row repeats;
 *     a segment whose rows are all excluded returns its first row M_b times, with NaN distances;
 *     squared distances in the subnormal range follow the device's denormal mode.
 *   One launch, one workgroup per segment.  A segment's ROUTE follows from its rows (d3d_fps_plan): routes 0 .. 2 keep coordinates and
 *   d in registers (three sizes), D3D_FPS_ROUTE_LDS adds LDS planes, D3D_FPS_ROUTE_STREAM (any size) reads the coordinates from global
 *   memory every step and keeps d in the workspace.  One launch may hold segments of every route; the bits do not depend on the route.
 *   Workspace: d3d_fps_workspace_bytes(n, segments, dtype).
 * d3d_fps_plan (pure host): the route a segment of segment_rows rows takes and the rows that route holds (2^31 - 1 for streaming).
 * d3d_ball_query: table[m, nsample] int32 and counts[m] int32.  point_offsets / center_offsets: DEVICE int64[segments + 1] as above
 *   (to n and to m), both or neither (NULL, NULL: one segment, `segments` ignored); a centre sees the points of its own segment only.
 *   The rule: r2 = r * r with r = radius rounded to the dtype; row i is inside iff q(i, c) < r2 -- strict, and false for NaN, so rows
 *   and centres that are not finite match nothing; the entries of a centre are the first nsample inside rows in ascending i (global
 *   row numbers), counts their number (at most nsample); the remaining slots are -1, or with pad_first != 0 the first entry again
 *   (pointnet2's convention; an empty ball stays -1 with count 0).  A table with -1 is what d3d_neighbor_gather and
 *   d3d_table_pool_forward read.  One launch, a wavefront per centre, O(m n) per segment; no workspace.
 * D3D_ERR_BAD_ARG: a negative size, a stride below 3, a missing pointer with work to do, nsample outside 1 .. 1024, a radius that is
 *   not a finite positive number, one offset array without the other; D3D_ERR_UNSUPPORTED: another dtype, n, m or segments above
 *   2^31 - 1; D3D_ERR_WORKSPACE: workspace missing or smaller than the query.  None of them launches anything.  segments == 0
 *   (sampling) and m == 0 (ball query) return D3D_OK before any HIP call. */
#define D3D_FPS_ROUTE_LDS 3
#define D3D_FPS_ROUTE_STREAM 4
size_t d3d_fps_workspace_bytes(int64_t n, int64_t segments, int32_t dtype);
int d3d_fps_plan(int64_t segment_rows, int32_t dtype, int32_t *route, int32_t *capacity);
int d3d_furthest_point_sample(const void *points, int64_t n, int32_t row_stride, int32_t dtype, const int64_t *point_offsets,
                              const int64_t *sample_offsets, int64_t segments, int64_t *indices, void *distances, void *workspace,
                              size_t workspace_bytes, void *stream);
int d3d_ball_query(const void *points, int64_t n, int32_t point_stride, const void *centers, int64_t m, int32_t center_stride, int32_t dtype,
                   const int64_t *point_offsets, const int64_t *center_offsets, int64_t segments, double radius, int32_t nsample,
                   int32_t pad_first, int32_t *table, int32_t *counts, void *stream);

/* The way back up (csrc/psample.hip, csrc/vinterp.hip): the k nearest known rows of every query row, their inverse-distance weights
 * and the weighted sum of their features -- three_nn / three_interpolate of pointnet2, the feature propagation of PointNet++, 3DSSD,
 * PV-RCNN's point heads; with a wider k the neighbourhoods of DGCNN and Point Transformer.  No atomics, no LDS, no workspace, nothing
 * waits on another wavefront, every run gives the same bits.  The reference has no counterpart.
 *
 * d3d_knn_query: d3d_ball_query's arguments with k in place of radius / nsample / pad: table[m, k] int32 and, where dist2 is not
 *   NULL, dist2[m, k] in `dtype`.  The rule, exact, with q(i, c) as above (every operation one rounding, no contraction):
 *     row i of the centre's own segment is a CANDIDATE iff q(i, c) is not NaN: rows and centres that are not finite by a NaN drop
 *       out (inf - inf is NaN as well); a q that overflows to +inf is a candidate and sorts last;
 *     the entries of a centre are its candidates in ascending (q, i): equal q resolves to the lower row first; entries are GLOBAL
 *       row numbers, dist2 holds the bits of their q;
 *     with fewer than k candidates the remaining slots are -1 / +inf; a NaN centre and an empty segment give -1 throughout;
 *     q in the subnormal range follows the device's denormal mode, as in d3d_furthest_point_sample.
 *   k in 1 .. D3D_KNN_MAX (the wave-sorted maximum: one held entry per lane).  One launch, a wavefront per centre, O(m n) per
 *   segment -- pointnet2's own cost, made for keypoint counts; no workspace.
 * d3d_knn_weights: table[m, k], dist2[m, k] (what d3d_knn_query wrote) -> weights[m, k] in `dtype`, power 1 or 2, eps >= 0 finite
 *   (rounded to the dtype first).  Per row, over the PRESENT entries (table >= 0) in ascending column:
 *     u_j = 1 / (sqrt(q_j) + eps) for power 1 (pointnet2's 1 / (dist + 1e-8)), u_j = 1 / (q_j + eps) for power 2;
 *     s = 0 + u_0 + u_1 + ..., w_j = u_j / s; absent entries get 0;
 *     all weights of the row are 0 when s == 0 or s is not finite -- that covers an exact hit with eps == 0 (u = +inf): give eps > 0
 *       where query rows may coincide with known rows.
 *   Every operation is one correctly rounded operation in the dtype (the build passes no fast-math flag; divide and sqrt are the
 *   correctly rounded ones).  One launch, one lane per row.
 * d3d_knn_interp_forward / d3d_knn_interp_backward: the signatures, rules and bits of d3d_table_interp_forward / _backward (above:
 *   out row = 0, then + (w * x) per present entry in ascending entry order, product and sum rounded separately, half types in fp32
 *   with one rounding at the store; backward through order / offsets of d3d_voxel_index over the flattened table) with the width j
 *   ANY value in 1 .. D3D_KNN_MAX, taken at run time -- the same kernel, its entries found through a run-time j.  For j == 1 and
 *   j == 8 the bits are those of d3d_table_interp_*.  feat[v, c]: the known rows; rows: the query rows.
 * D3D_ERR_BAD_ARG: a negative size, a stride below 3, k (j) < 1, c < 1, one offset array without the other, a power other than 1 or
 *   2, an eps that is negative or not finite, a missing pointer with work to do; D3D_ERR_UNSUPPORTED: another dtype (query and
 *   weights: D3D_F32 / D3D_F64; the folds also D3D_F16 / D3D_BF16), n, m, v or segments above 2^31 - 1, m * k (rows * j) above
 *   2^31 - 1 for the weights and the folds, k (j) above D3D_KNN_MAX.  None of them launches anything.  m == 0 (query, weights),
 *   rows == 0 (forward) and v == 0 (backward) return D3D_OK before any HIP call. */
#define D3D_KNN_MAX 64
int d3d_knn_query(const void *points, int64_t n, int32_t point_stride, const void *centers, int64_t m, int32_t center_stride, int32_t dtype,
                  const int64_t *point_offsets, const int64_t *center_offsets, int64_t segments, int32_t k, int32_t *table, void *dist2,
                  void *stream);
int d3d_knn_weights(const int32_t *table, const void *dist2, int64_t m, int32_t k, int32_t dtype, int32_t power, double eps, void *weights,
                    void *stream);
int d3d_knn_interp_forward(const void *feat, int64_t v, int32_t c, int32_t dtype, const int32_t *table, const void *weights, int64_t rows,
                           int32_t j, void *out, void *stream);
int d3d_knn_interp_backward(const void *grad, int64_t rows, int32_t c, int32_t dtype, const int32_t *order, const int64_t *offsets,
                            const void *weights, int32_t j, int64_t v, void *grad_feat, void *stream);

/* ------------------------------------------------------------------ PointGrid: grid-accelerated ball query and kNN, the same bits */

/* A uniform cell index of a cloud, built once per frame, and the two neighbour searches over it (csrc/pgrid.hip).  d3d_ball_query_grid
 * and d3d_knn_query_grid return BIT FOR BIT what d3d_ball_query / d3d_knn_query return for the same points, centres and arguments --
 * tables, counts, dist2, padding, -1 / +inf tails, GLOBAL row numbers -- and read only the cells a centre can reach (the proofs:
 * DESIGN.md 8j).  No float atomics, no LDS; the queries take no workspace.  The reference has no counterpart.
 *
 * The grid, per SEGMENT (one cloud, or one slice of point_offsets):
 *   a FINITE ROW has three finite coordinates.  lo_a / hi_a = the least / largest coordinate a over the segment's finite rows, as
 *     doubles (exact for fp32); a segment without a finite row has lo = 0 and ONE cell;
 *   cap = max(64, ceil(max_cells_per_point * finite rows)) as a double: a bound on memory (offsets: 8 bytes per cell), not a tuning
 *     number, and what keeps a cloud with int32-sized or 1e19 coordinates legal;
 *   h = the first of cell_size * 2^j, j = 0, 1, ..., with prod_a (floor((hi_a - lo_a) / h) + 1) <= cap, the quotients and the product
 *     in fp64, compared BEFORE any conversion to an integer; inv_h = 1 / h in fp64; dim_a = floor((hi_a - lo_a) * inv_h) + 1;
 *   the cell of a coordinate: cell_a(x) = clamp(floor((fp64(x) - lo_a) * inv_h), 0, dim_a - 1), clamped while still a double; a NaN
 *     gives 0 (centres only).  Every step is monotone in x, so cell_a is: all that follows rests on that;
 *   cell id = base_s + (z * dim_y + y) * dim_x + x: x is fastest, so the cells of an x range at fixed (y, z) are ONE contiguous run
 *     of `order`;
 *   a row with a NaN coordinate maps to -1 (it can be a candidate of neither query); a row without NaN but with an infinite
 *     coordinate maps to the segment's OVERFLOW CELL base_s + dim_x * dim_y * dim_z (d3d_knn_query counts q = +inf as a candidate
 *     that sorts last: these rows stay reachable); base_0 = 0, base_{s+1} = base_s + cells_s + 1; total_cells = the sum, at most
 *     2^31 - 1;
 *   order / offsets = d3d_voxel_index(mapping, n, total_cells), unchanged: rows grouped by cell, ascending row inside a cell;
 *   packed[K', 3] in `dtype`: the coordinates of row order[j] at entry j, K' = counts[0] = the mapped rows.
 *
 * d3d_point_grid_bounds: points[n, row_stride >= 3] as d3d_ball_query reads them; point_offsets: DEVICE int64[segments + 1] or NULL
 *   (one segment, `segments` ignored) -> DEVICE bounds[S, 6] = (lo_x, lo_y, lo_z, hi_x, hi_y, hi_z) as doubles and finite_rows[S]
 *   int64, zeros for a segment without a finite row.  Integer atomic maxima on order-keeping keys and an integer sum: the same bits on
 *   every run.  The caller reads both back (ONE host read-back per grid) for
 * d3d_point_grid_plan (PURE HOST, no HIP call): HOST bounds, finite_rows -> HOST plan[S] and *total_cells.  cell_size and
 *   max_cells_per_point: finite, > 0.  D3D_ERR_UNSUPPORTED: total_cells above 2^31 - 1, an extent hi - lo that is not finite.
 * d3d_point_grid_build: DEVICE plan[S] -> mapping[n] int64, then order[n] int32, offsets[total_cells + 1] int64 and counts[2] int64
 *   exactly as d3d_voxel_index writes them (its launches, its workspace: d3d_point_grid_workspace_bytes(n, total_cells)), then
 *   packed.  point_offsets as above, TRUSTED.
 * d3d_ball_query_grid / d3d_knn_query_grid: the centres, radius / nsample / pad_first or k, table, counts or dist2 of d3d_ball_query /
 *   d3d_knn_query, and the grid in place of the points: n (its rows), plan, order, cell_offsets (= offsets), packed, all DEVICE and
 *   TRUSTED.  center_offsets: DEVICE int64[segments + 1], required iff the grid was built with point_offsets (NULL: one segment); a
 *   centre sees the cells of its own segment only.  One launch, a wavefront per centre.
 *     ball: the box of cells of u_a - R .. u_a + R per axis, u_a = fp64(x_c) - lo_a, R = r (1 + 2^-20), every edge moved outward by
 *       2^-50 of itself; the entries are the nsample LOWEST rows among the inside rows of the box -- the first nsample inside rows in
 *       ascending row, as d3d_ball_query's.  The overflow cell is never read.
 *     kNN: rings of cells around the centre's own clamped cell; after ring rho, d = the least distance of the centre to a face of
 *       the walked box that is not on the grid's border (faces at j * h, the centre at u_a), dd = d (1 - 2^-20) - 2^-20 h; the
 *       walk ends iff the k-th held key exists and fp64(q_k) < dd * dd * (1 - 2^-20), with dd > 0 and the right side at least four
 *       times the smallest normal number of the dtype -- STRICT: an unexplored row with equal q and a lower row number would win the
 *       tie.  When every face is on the border the grid is exhausted; the overflow cell is walked then unless the k-th key is
 *       there with a finite q.
 *   nsample and k are at most D3D_KNN_MAX here (one held entry per lane): above it D3D_ERR_UNSUPPORTED -- d3d_ball_query takes up to
 *   1024.
 * D3D_ERR_BAD_ARG: a negative size, a stride below 3, nsample / k below 1 (nsample above 1024), a radius, cell_size or
 *   max_cells_per_point that is not a finite positive number, bounds that are not finite or not ordered, total_cells < 1, a missing
 *   pointer with work to do; D3D_ERR_UNSUPPORTED: another dtype than D3D_F32 / D3D_F64, n, m, segments or total_cells above 2^31 - 1,
 *   nsample / k above D3D_KNN_MAX; D3D_ERR_WORKSPACE: workspace missing or smaller than the query.  None of them launches anything.
 *   m == 0 (queries) and S == 0 (bounds, plan) return D3D_OK before any HIP call. */
typedef struct D3DPointGridSegment {
    double lo[3];
    double h, inv_h;
    int64_t base;      /* the id of the segment's first cell; its overflow cell is base + dim[0] * dim[1] * dim[2] */
    int32_t dim[3];
    int32_t pad_;
} D3DPointGridSegment; /* 64 bytes */
int d3d_point_grid_bounds(const void *points, int64_t n, int32_t row_stride, int32_t dtype, const int64_t *point_offsets, int64_t segments,
                          double *bounds, int64_t *finite_rows, void *stream);
int d3d_point_grid_plan(const double *bounds, const int64_t *finite_rows, int64_t segments, double cell_size, double max_cells_per_point,
                        D3DPointGridSegment *plan, int64_t *total_cells);
size_t d3d_point_grid_workspace_bytes(int64_t n, int64_t total_cells);
int d3d_point_grid_build(const void *points, int64_t n, int32_t row_stride, int32_t dtype, const int64_t *point_offsets, int64_t segments,
                         const D3DPointGridSegment *plan, int64_t total_cells, int64_t *mapping, int32_t *order, int64_t *offsets,
                         int64_t *counts, void *packed, void *workspace, size_t workspace_bytes, void *stream);
int d3d_ball_query_grid(const void *centers, int64_t m, int32_t center_stride, int32_t dtype, const int64_t *center_offsets, int64_t segments,
                        const D3DPointGridSegment *plan, const int32_t *order, const int64_t *cell_offsets, const void *packed, int64_t n,
                        double radius, int32_t nsample, int32_t pad_first, int32_t *table, int32_t *counts, void *stream);
int d3d_knn_query_grid(const void *centers, int64_t m, int32_t center_stride, int32_t dtype, const int64_t *center_offsets, int64_t segments,
                       const D3DPointGridSegment *plan, const int32_t *order, const int64_t *cell_offsets, const void *packed, int64_t n,
                       int32_t k, int32_t *table, void *dist2, void *stream);

/* ------------------------------------------------------------------ RoI pooling of points: the cell table of rotated boxes */

/* The step where a two-stage detector turns a proposal box back into features (csrc/roipool.hip, csrc/vtpool.hip): the points inside
 * every rotated box, binned into the cells of the box's own grid -- Part-A2's roiaware_pool3d (its pts_idx_of_voxels), and with one cell
 * and the cyclic fill PointRCNN's roipoint_pool3d.  The table is a -1-padded int32 table like d3d_ball_query's: d3d_table_pool_forward
 * folds it, d3d_table_pool_backward_index is that fold's gradient.  No float atomics, no [m, n] mask, no sort, no workspace; every
 * run gives the same bits.  The reference has crop_points and nothing that bins.
 *
 * d3d_roi_grid_table: points[n, point_stride >= 3] and box row i = 7 floats (x, y, z, lx, ly, lz, rz; z the centre) at boxes + i *
 *   box_stride + box_offset, exactly as d3d_crop_3dr reads them; dtype D3D_F32 only.  point_offsets / box_offsets: DEVICE
 *   int64[segments + 1] as d3d_ball_query's (to n and to m), both or neither, trusted; a box sees the points of its own segment only.
 *   out_size: HOST int32[3] = (ox, oy, oz), G = ox * oy * oz cells; max_points = P; pad 0 or 1.  ->
 *     table[m, G, P] int32: GLOBAL point rows, -1 for none;  counts[m, G] int32: the kept entries (<= P);
 *     inside[m] int32: all members of the box, uncapped.
 *   The rule.  All arithmetic is fp32, every operation one rounding (the build does not contract).
 *     MEMBER: point i belongs to box b iff its x, y and z are all finite AND the test of d3d_crop_3dr holds -- the same function on the
 *       same expressions (contains3 of csrc/geom.hpp), so for finite points the result is d3d_crop_3dr's bits.  A NaN z, which
 *       d3d_crop_3dr counts as inside, is excluded here: no cell can be computed for it.  A box row on which that test is false for
 *       every point (NaN fields, degenerate extents) has no members.  ONE predicate decides membership; the cell never does.
 *     CELL: with (s, c) = the sine and cosine d3d_crop_3dr takes of rz (the host's sinf / cosf), dx = x - bx, dy = y - by, dz = z - bz:
 *         u = dx * c + dy * s,  v = dy * c - dx * s,
 *         t_x = (u / lx + 0.5f) * ox,  t_y = (v / ly + 0.5f) * oy,  t_z = (dz / lz + 0.5f) * oz   (ox, oy, oz as floats),
 *         i_a = 0 where !(t_a >= 0) -- a NaN t maps to cell 0 --, else min(trunc(t_a), o_a - 1), saturated BEFORE the conversion,
 *         cell = (i_x * oy + i_y) * oz + i_z.
 *       The cells are CLAMPED: a member on a face whose t lands at o_a, or a hair outside, falls into the border cell.
 *     ENTRIES: a cell's entries are its first P members in ascending global row, counts is their number, the remaining slots are -1.
 *       pad == 1 ("cycle", PointRCNN's fill): slot j >= count holds entry j % count; an empty cell stays -1 with count 0.
 *   Nothing of this depends on the launch shape: d3d_roi_grid_plan's numbers say where the kernel's seams lie, not what it computes.
 *   One launch, one workgroup per box, O(m n) per segment as d3d_ball_query; every slot of the table is written exactly once by that
 *   launch (no memset).  P in 1 .. 1024; G <= d3d_roi_grid_max_cells(); m * G * P, n, m and segments at most 2^31 - 1.
 * d3d_roi_grid_max_cells (pure host): the largest G, 4096 = 16^3.
 * d3d_roi_grid_plan (pure host): for a segment of segment_rows rows and a grid of `cells` cells, what the launch uses: tile_rows,
 *   the rows one ballot judges; slab_rows, the contiguous rows one wavefront judges at a time (slab k = rows [k * slab_rows, (k + 1) *
 *   slab_rows) of the segment; its members wait in on-chip memory, which holds a whole slab); round_rows, the rows the workgroup
 *   takes between two barriers, a whole number of slabs -- the members of a round are placed before the next round is loaded.
 * d3d_table_pool_backward_index: the gradient of d3d_table_pool_forward for a table that has no fixed-width transposed table (a point
 *   lies in as many boxes as overlap it).  grad_out[rows, c] in `dtype`, the forward's table [rows, k] given as its inverted index:
 *   order[offsets[v] .. offsets[v + 1]) names, for source row v, the entries e = r * k + kk that hold v, in ascending e (DEVICE int32 /
 *   int64[src_rows + 1], trusted: d3d_knn_interp_backward's layout) -> grad_feat[src_rows, c].  Entry e contributes grad_out[r] (SUM),
 *   grad_out[r] / (T)count[r] (MEAN), grad_out[r, ch] where arg[r, ch] == kk and nothing elsewhere (MAX / MIN); the contributions are
 *   added to 0 in ascending e.  D3D_F16 / D3D_BF16: contributions and sum in fp32, one rounding.  Every row of grad_feat is written
 *   exactly once, zero where nothing names it.  arg [rows, c] int16 and count [rows] int32 as the forward wrote them (arg read for
 *   MAX / MIN only, count for MEAN only).  16-byte row moves under d3d_table_pool_backward's conditions, the same bits on both paths.
 *   dtype D3D_F32, D3D_F64, D3D_F16 or D3D_BF16; c >= 1; k in 1 .. 343; src_rows and rows * k at most 2^31 - 1.  One launch.
 * D3D_ERR_BAD_ARG: a negative size, a stride below 3 (box_stride below box_offset + 7), a missing pointer with work to do, one offset
 *   array without the other, an out_size component below 1, P outside 1 .. 1024, a pad other than 0 or 1, c < 1, k < 1;
 *   D3D_ERR_UNSUPPORTED: the limits above, another dtype or reduction code.  None of them launches anything.  m == 0 (table) and
 *   src_rows == 0 (backward) return D3D_OK before any HIP call. */
int32_t d3d_roi_grid_max_cells(void);
int d3d_roi_grid_plan(int64_t segment_rows, int32_t cells, int32_t *tile_rows, int32_t *slab_rows, int32_t *round_rows);
int d3d_roi_grid_table(const void *points, int64_t n, int32_t point_stride, const void *boxes, int64_t m, int32_t box_stride,
                       int32_t box_offset, int32_t dtype, const int64_t *point_offsets, const int64_t *box_offsets, int64_t segments,
                       const int32_t *out_size, int32_t max_points, int32_t pad, int32_t *table, int32_t *counts, int32_t *inside,
                       void *stream);
int d3d_table_pool_backward_index(const void *grad_out, int64_t rows, int32_t c, int32_t dtype, const int32_t *order, const int64_t *offsets,
                                  int64_t src_rows, int32_t k, int32_t reduction, const int16_t *arg, const int32_t *count,
                                  void *grad_feat, void *stream);

/* ------------------------------------------------------------------ camera features to voxel rows: the frustum map and lift-splat */

/* The "lift, splat" view transform of LSS / BEVDet / BEVDepth / BEVFusion (bev_pool), csrc/vlift.hip: every pixel of S = B * N cameras
 * carries a depth distribution over D bins and a context row of C channels; the K = S * D * H * W frustum points are placed in the ego
 * grid and every cell gets the sum of depth[p] * feat[pixel(p)] over its points.  The result is voxel rows [V, C] with coords, as the
 * voxelizer's: d3d_vdense_scatter is the dense exit, the sparse convolutions take the rows as they are.  No float atomics, the [K, C]
 * product never exists, every run gives the same bits.  The reference has no counterpart.
 *
 * d3d_frustum_map_count: DEVICE fp32 arrays us[w] (pixel columns), vs[h] (pixel rows), ds[d] (depth bins) -- given explicitly, no
 *   linspace rounding is part of the contract --, pre[s, 3, 4] and post[s, 3, 4] row-major; HOST arrays lo[3], size[3] fp32 and
 *   shape[3] int32 in coordinate-column order (x, y, z) as the voxelizer's coords; cams_per_sample = N.
 *   Point p = ((cam * D + d) * H + h) * W + w.  Every operation below is ONE rounding in fp32 (the build does not contract):
 *     a   = (us[w], vs[h], ds[d])
 *     q_i = ((pre[i,0] * a0 + pre[i,1] * a1) + pre[i,2] * a2) + pre[i,3]
 *     e   = (q0 * q2, q1 * q2, q2)
 *     x_i = ((post[i,0] * e0 + post[i,1] * e1) + post[i,2] * e2) + post[i,3]
 *     t_i = (x_i - lo_i) / size_i
 *   The point is a MEMBER iff t_i >= 0 && t_i < shape_i on all three axes (a NaN fails; -0.0 passes and lands in cell 0); its
 *   coordinate is c_i = (int32) t_i, its sample b = cam / N.  Points with t in (-1, 0) are NOT members: the .long() truncation of
 *   LSS's voxel_pooling rounds that band toward zero and folds it into cell 0 -- this rule does not, deliberately.
 *   Present cells are numbered by ascending key ((b * n0 + c0) * n1 + c1) * n2 + c2: the numbering is a function of the input alone.
 *   _count writes, into the workspace, the per-point key, the marks of the present cells (a bitmap, set with integer atomics) and
 *   their scan; counts[2] int64 = {V, the members}.  The caller reads counts back, allocates and calls
 * d3d_frustum_map_emit with the SAME workspace, untouched in between, and the same sizes: mapping[K] int64 (the row of every point, -1
 *   for none), coords[v, 3] int64 (x, y, z) and batch_index[v] int64, rows in ascending key.  v is the V of _count (rows from v on are
 *   not written).  The inverted index (order, offsets) of the folds is d3d_voxel_index(mapping, K, V), unchanged.
 *   Launches: cells, the scan trio (count), rows, coords (emit); every dependency is a kernel boundary, nothing waits on another
 *   workgroup.  Workspace: d3d_frustum_map_workspace_bytes(K, B * n0 * n1 * n2), caller-owned.
 *   D3D_ERR_BAD_ARG: a size[i] that is not positive or not finite, a shape[i] below 1, cams_per_sample below 1, s % cams_per_sample
 *   != 0, a negative size, v above the number of cells, a missing pointer; D3D_ERR_UNSUPPORTED: K or B * n0 * n1 * n2 above 2^31 - 1;
 *   D3D_ERR_WORKSPACE: workspace missing or smaller than the query.  All refusals come before any HIP call.
 *
 * The folds.  depth[s, d, h, w] and feat[s, h, w, c] (channels-last) in ONE dtype: D3D_F32, D3D_F64, D3D_F16 or D3D_BF16; the half
 *   types multiply and add in fp32 and round once, to nearest even, at the store.  pix(p) = (p / (D * H * W)) * H * W + p % (H * W).
 *   Rows move as 16-byte vectors when c is a multiple of 4 (f32) / 2 (f64) / 8 (f16, bf16) and the row pointers are 16-byte aligned,
 *   element by element otherwise: the same bits on both paths.  One launch each, no workspace, nothing read back.
 * d3d_lift_pool_forward: out[r] is 0, then + (depth[p] * feat[pix(p)]) for p in order[offsets[r] .. offsets[r + 1]) in that order --
 *   the product and the sum are two roundings.  out[v, c], every row written exactly once (a row without points: 0).  order / offsets
 *   as d3d_voxel_index wrote them (trusted).  One lane group per row, eight feature rows in flight; a crowded cell is a long
 *   sequential fold by contract.
 * d3d_lift_pool_backward_feat: grad_feat[pixel] is 0, then + (depth[p] * grad[mapping[p]]) over d = 0 .. D - 1 ascending for the
 *   points p of that pixel with mapping[p] in [0, v).  A gather: grad_feat[s, h, w, c], every row written exactly once; needs no index.
 * d3d_lift_pool_backward_depth: grad_depth[p] = sum over ch of grad[mapping[p], ch] * feat[pix(p), ch], 0 where mapping[p] is not in
 *   [0, v).  Products and sums in fp32 (fp64 for D3D_F64), every product rounded, reduced across the lane group; the ORDER of the sum
 *   is the kernel's own: |result - exact| <= (c + 1) * u * sum |grad * feat| (u the unit roundoff of the accumulation type) plus the
 *   one rounding of the store.  This is the one output that is not defined bit for bit; it is still the same bits on every run.
 *   D3D_ERR_BAD_ARG: a negative size, c < 1, a missing pointer with work to do; D3D_ERR_UNSUPPORTED: another dtype, K, v (and for
 *   _backward_feat s * h * w) above 2^31 - 1.  None of them launches anything.  v == 0 (forward), s * h * w == 0 (_backward_feat) and
 *   K == 0 (_backward_depth) return D3D_OK before any HIP call. */
size_t d3d_frustum_map_workspace_bytes(int64_t k, int64_t cells);
int d3d_frustum_map_count(const float *us, int32_t w, const float *vs, int32_t h, const float *ds, int32_t d, const float *pre,
                          const float *post, int64_t s, int32_t cams_per_sample, const float *lo, const float *size, const int32_t *shape,
                          int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int d3d_frustum_map_emit(int32_t w, int32_t h, int32_t d, int64_t s, int32_t cams_per_sample, const int32_t *shape, int64_t v,
                         int64_t *mapping, int64_t *coords, int64_t *batch_index, void *workspace, size_t workspace_bytes, void *stream);
int d3d_lift_pool_forward(const void *depth, const void *feat, int64_t s, int32_t d, int32_t h, int32_t w, int32_t c, int32_t dtype,
                          const int32_t *order, const int64_t *offsets, int64_t v, void *out, void *stream);
int d3d_lift_pool_backward_feat(const void *grad, int64_t v, const void *depth, const int64_t *mapping, int64_t s, int32_t d, int32_t h,
                                int32_t w, int32_t c, int32_t dtype, void *grad_feat, void *stream);
int d3d_lift_pool_backward_depth(const void *grad, int64_t v, const void *feat, const int64_t *mapping, int64_t s, int32_t d, int32_t h,
                                 int32_t w, int32_t c, int32_t dtype, void *grad_depth, void *stream);

/* ------------------------------------------------------------------ the centre head: peaks of a heat map, circle NMS, target drawing */

/* The station between the BEV map and the boxes in CenterPoint, BEVFusion, BEVDet, PillarNet and OpenPCDet's CenterHead,
 * csrc/center.hip.  The reference has no counterpart.  Every output is integers, copies of input bits or one rounded expression; no
 * float atomics, the same bits on every run, nothing is read back to the host, and no launch waits on another workgroup.
 *
 * d3d_heatmap_peaks: CenterNet's _nms + _topk (max_pool2d(heat, kernel, 1, kernel / 2) == heat, multiply, topk over C * H * W;
 *   OpenPCDet's centernet_utils._topk: two topk's) on heat[b, c, h, w], contiguous, D3D_F32, D3D_F16 or D3D_BF16, read only.
 *   PEAK: cell (b, c, y, x) is a peak iff no value in its kernel x kernel window -- clipped to the plane, inside the cell's own class
 *     plane -- is NaN and its value is >= every value of the window.  That is max_pool2d == heat exactly, NaN and +-inf included.
 *     kernel 1: every cell that is not NaN.  -0.0 == +0.0.  Every cell of a plateau is a peak.
 *   CANDIDATE: a peak whose value, widened to fp32 (exact for the half types), is > threshold (fp32; has_threshold == 0: every peak,
 *     -inf included).
 *   RANKING: by descending value in the order of csrc/lds_sort.hpp's KeyBits<float>::desc on the widened value, so equal values, and
 *     -0 against +0, are ties; ties go to the lowest flat index (c * h + y) * w + x.  (torch.topk leaves the tie order open.)
 *   -> scores[b, k] in heat's dtype: the INPUT'S OWN BITS of the k best candidates in ranking order (-0.0 comes back as -0.0),
 *     -inf in the missing slots; classes, ys, xs [b, k] int32, -1 in the missing slots; counts[b] int32 = min(k, candidates).
 *   No sigmoid inside: it is monotone, the caller applies it to the [b, k] scores; peaks and ties are those of the values passed in.
 *   How: an exact radix select on the 32-bit key.  Three counting passes over the map (the top 12 key bits, the next 12 inside the
 *   pivot bin, the last 8: per-workgroup histograms in on-chip memory, flushed with integer atomics), each followed by one workgroup
 *   per sample that walks the histogram; then the k-th key and the number of candidates strictly above it are known.  A count pass,
 *   a scan per sample and an emit pass compact the candidates above the pivot key and, of those equal to it, the `need` lowest flat
 *   indices (a workgroup owns 1024 consecutive flat cells, so the order of the ties is a prefix sum).  One workgroup per sample
 *   orders the <= k winners on (key, flat index), a unique composite.  Every pass recomputes the peak test from the map; no
 *   [b, c, h, w] intermediate exists.  A constant map and any other map cost the same five passes.  Eleven launches and one memset.
 *   Workspace: d3d_heatmap_peaks_workspace_bytes(b, c, h, w, k) = O(b * (3 * 4096 bins + c * h * w / 1024 tiles + k)) bytes.
 *   Limits: c * h * w <= 2^31 - 1, b <= 65535, k in 1 .. d3d_heatmap_peaks_max() = 4096, kernel in {1, 3, 5, 7}.  Sample offsets
 *   b * c * h * w are 64-bit.
 *   D3D_ERR_BAD_ARG: a negative b, c, h or w below 1, k below 1, another kernel, has_threshold not 0 or 1, a missing pointer with
 *   b > 0; D3D_ERR_UNSUPPORTED: another dtype, the limits above (the size query returns 0 for them); D3D_ERR_WORKSPACE: workspace
 *   missing or smaller than the query.  All refusals come before any HIP call; b == 0 returns D3D_OK.
 *
 * d3d_circle_nms: det3d's circle_nms (core/utils/circle_nms_jit.py, a numba loop on the host; OpenPCDet copies to the host for it)
 *   inside every segment of a batch and never across segments.  centers: rows of `stride` >= 2 elements, columns 0 and 1 = (x, y);
 *   scores[n]; D3D_F32 or D3D_F64, both in one dtype.  Segment s is rows perm[seg_offsets[s] .. seg_offsets[s + 1]) (DEVICE int64
 *   arrays, trusted; perm NULL: the rows seg_offsets[s] .. themselves).  max_segment: the longest segment, given by the caller.
 *   Inside a segment the rows are visited in d3d_argsort_desc's order -- descending score, NaN first, ties in ascending position in
 *   the segment (ascending row for a stable perm).  A visited row that is not suppressed is kept; a kept row i suppresses every
 *   later row j with  d2 = (xi - xj) * (xi - xj) + (yi - yj) * (yi - yj) <= t,  every operation rounded once in the dtype (the build
 *   does not contract), t = dist2_threshold rounded to the dtype -- the SQUARED distance (CenterPoint's configs pass their "radius"
 *   straight into this slot).  A NaN d2 suppresses nothing; a suppressed row suppresses nothing.  max_keep (CenterPoint's
 *   post_max_size): only the first max_keep kept rows of a segment, in visiting order, stay.  -> keep[n] u8, indexed by ROW: every
 *   byte of a segment's rows is written exactly once, 1 = kept; rows of no segment and empty segments are not touched.
 *   One launch, one workgroup per segment, everything on chip, no atomics: the segment is sorted (sort_lds), then swept in blocks
 *   of 64 ranks -- one wavefront resolves a block (one ballot per open row), all wavefronts apply its kept rows to the later ranks.
 *   D3D_ERR_BAD_ARG: a negative size, stride < 2, max_keep < 0, a missing pointer with work to do; D3D_ERR_UNSUPPORTED: another
 *   dtype, max_segment above d3d_circle_nms_max() = 4096, n or segments above 2^31 - 1.  A segment longer than max_segment is
 *   skipped by its workgroup untouched.  n == 0, segments == 0 and max_segment == 0 return D3D_OK before any HIP call.
 *
 * d3d_gaussian_heatmap: CenterNet's draw_umich_gaussian for every box of a batch (OpenPCDet: draw_gaussian_to_heatmap once per box
 *   from a Python loop) -> out[b, c, h, w] fp32.  centers[m, 2] int32 = (x, y) = (column, row), anywhere, outside the map too;
 *   radii[m] int32 in 0 .. 4095 and classes[m] int32 (trusted: the caller has checked them; a class outside [0, c) draws nothing);
 *   offsets: DEVICE int64[b + 1], the boxes of every sample, or NULL with b == 1.
 *     out[s, cl, y, x] = the maximum of 0 and, over the boxes i of sample s with classes[i] == cl, |x - cx| <= r and |y - cy| <= r, of
 *         g(r, d2) = (float) exp( -(double)(18 * d2) / (double)((2 r + 1) * (2 r + 1)) ),   d2 = (x - cx)^2 + (y - cy)^2:
 *   gaussian2D with sigma = (2 r + 1) / 6 over the SQUARE window, clipped at the borders.  The integers are exact; then one fp64
 *   division, one fp64 exp (the device library's, within 1 ulp) and one rounding to fp32.  The centre cell is exactly 1.0.
 *   CenterNet's `h < eps * max` mask never fires and is left out: d2 <= 2 r^2 keeps the exponent above -9, and e^-9 = 1.2e-4 is far
 *   above fp32's eps.  One launch: a workgroup owns a 16 x 64 tile of one class plane and takes the sample's boxes through on-chip
 *   memory 256 at a time, dropping by ballot those of another class or whose window misses the tile; every element of out is stored
 *   exactly once, zeros included -- no memset, no atomics.
 *   D3D_ERR_BAD_ARG: a negative size, offsets NULL with b > 1, a missing pointer with work to do; D3D_ERR_UNSUPPORTED: b or c above
 *   65535, h or w above 2^30, m above 2^31 - 1.  An empty out returns D3D_OK before any HIP call. */
int32_t d3d_heatmap_peaks_max(void);
size_t d3d_heatmap_peaks_workspace_bytes(int64_t b, int64_t c, int64_t h, int64_t w, int32_t k);
int d3d_heatmap_peaks(const void *heat, int64_t b, int64_t c, int64_t h, int64_t w, int32_t dtype, int32_t k, int32_t kernel,
                      int32_t has_threshold, float threshold, void *scores, int32_t *classes, int32_t *ys, int32_t *xs, int32_t *counts,
                      void *workspace, size_t workspace_bytes, void *stream);
int32_t d3d_circle_nms_max(void);
int d3d_circle_nms(const void *centers, int32_t stride, const void *scores, const int64_t *perm, const int64_t *seg_offsets, int64_t n,
                   int64_t segments, int32_t max_segment, int32_t dtype, double dist2_threshold, int32_t max_keep, uint8_t *keep,
                   void *stream);
int d3d_gaussian_heatmap(const int32_t *centers, const int32_t *radii, const int32_t *classes, const int64_t *offsets, int64_t m,
                         int64_t b, int64_t c, int64_t h, int64_t w, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* D3D_HIP_H */
