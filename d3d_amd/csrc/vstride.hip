// vstride.hip -- the map of a strided sparse convolution on MI355X (gfx950): from the active input voxels to the active OUTPUT voxels
// of a convolution with a kernel size, stride, padding and dilation per axis, and the two tables that relate their rows.  What the
// downsampling layers of a voxel backbone (SECOND, CenterPoint, PV-RCNN) and the inverse convolutions of a sparse U-Net need before
// their GEMM.  An extension: the reference stops at the voxelizer.
//
//   d3d_sparse_conv_map_count  coords[V,3] (+ batch[V]) -> counts = {Vout, entries, 0, span overflow, input outside spatial_shape}
//   d3d_sparse_conv_map_emit   ... -> out_coords[Vout,3], out_batch[Vout], table_in[V,K], table_out[Vout,K], counts[2] = duplicates
//
// Input i feeds output o through column k = (ix ky + iy) kz + iz when o * stride - padding + (ix,iy,iz) * dilation == i on every
// axis; a pair (v, k) of an input row and a column that has such an o is a CANDIDATE, numbered c = v K + k.  Output rows are numbered
// in the order of their FIRST candidate.  The launches, every dependency a kernel boundary (no workgroup waits on another):
//   k_vn_bounds       min / max of every input axis and of the batch value (vkey.hpp, shared with vnbr.hip, as the table is)
//   k_sc_frame        one lane: the output box from the bounds (clipped by spatial_shape), its spans, the verdicts, the table's capacity
//   k_sc_clear        the slots {key, first} of the open-addressing table <- all ones
//   k_sc_insert       one lane per (v, k): the key of o over the OUTPUT box, the claim of its slot (vkey.hpp), then a 64-bit integer
//                     atomicMin of c on the slot's second word: the winner is the first candidate whatever order the lanes arrive in
//   k_scan_count / k_scan_bsum (common.hpp) over the marks "c is its slot's minimum"  -> Vout               ... the host reads counts
//   k_scan_apply      the first candidates write out_coords, out_batch and their row number into their slot
//   k_sc_tables       one lane per (v, k), the column fastest: table_in[v,k] = row (-1: no candidate; contiguous stores), and the
//                     claim of table_out[row,k] by an integer atomicCAS -1 -> v; a failed claim = two inputs on one (batch, coordinate)
// Integer atomics only; the same result on every run.
#include <algorithm>
#include "vkey.hpp"
#include "vrow.hpp"                                    // (the row limit)

namespace {

constexpr int64_t kScBlocks = 1ll << 24;
constexpr int kScClearBlocks = 4096;
constexpr int32_t kScMaxStep = 1 << 24;                // stride, padding, dilation: their sums with a position stay far inside int64
constexpr int64_t kScMaxShape = 0x7fffffffll;

struct alignas(16) ScSlot {
    unsigned long long key, first;                     // first: the smallest candidate number so far; after k_scan_apply the output row
};

struct ScShape {
    int32_t k[3], s[3], p[3], d[3];
    int32_t has_shape;
    int64_t in[3], out[3];                             // spatial_shape and dense conv3d's output size for it
};

// what k_sc_frame derives from the measured bounds, read by every later launch
struct ScFrame {
    unsigned long long ilo[4];       // the smallest input value per axis and the smallest batch value (bits of the int64)
    unsigned long long olo[3];       // the first output coordinate of the box per axis (bits of the int64)
    unsigned long long span[4];      // the output box per axis (0: empty) and the batch span
    int64_t base[3];                 // position in the box = (base + (i - ilo) - ix * dilation) / stride, where that divides
    int32_t log2cap, refused;
};

struct ScWs {
    unsigned long long *bounds;      // [4][2], as in vnbr.hip
    ScFrame *frame;
    ScSlot *slots;
    unsigned long long *bsum;        // the scan's block sums: exclusive after d3d_sparse_conv_map_count, read by _emit
    int log2cap;                     // of the allocation; the launches use the frame's, which is never larger
};
// the one layout: carved here for both entries, and on a null base for the size query.  vp = V * P bounds the distinct outputs
ScWs sc_carve(WsCarver &w, int64_t vp, int64_t n)
{
    ScWs r;
    r.log2cap = nbr_log2cap((unsigned long long)vp);
    r.bounds = w.take<unsigned long long>(8);
    r.frame = w.take<ScFrame>(1);
    r.slots = w.take<ScSlot>((size_t)1 << r.log2cap);
    r.bsum = w.take<unsigned long long>((size_t)std::max<int64_t>(d3d_divup(n, kScanTile), 1));
    return r;
}

__host__ __device__ inline int64_t sc_floordiv(int64_t a, int64_t b)      // b > 0
{
    const int64_t q = a / b;
    return q * b > a ? q - 1 : q;
}

int64_t sc_gcd(int64_t a, int64_t b) { return b ? sc_gcd(b, a % b) : a; }

// P: the largest number of outputs one input can feed, the product over the axes of ceil(k / (s / gcd(s, d))): on an axis the
// columns ix that reach an output from one input are those with ix * d = i + p (mod s), every (s / gcd(s, d))-th one
int64_t sc_fanout(const ScShape &s)
{
    int64_t p = 1;
    for (int a = 0; a < 3; a++) p *= d3d_divup(s.k[a], s.s[a] / sc_gcd(s.s[a], s.d[a]));
    return p;
}

__global__ void k_sc_frame(const unsigned long long *__restrict__ bounds, int has_batch, ScShape s, int64_t vp, ScFrame *__restrict__ frame,
                           int64_t *__restrict__ counts)
{
    if (blockIdx.x || threadIdx.x) return;
    ScFrame f;
    bool overflow = false, outside = false, empty = false;
#pragma unroll                                                                            // (static indices: the frame stays in registers)
    for (int a = 0; a < 3; a++) {
        unsigned long long lo, hi;
        nbr_axis(bounds, a, lo, hi);
        const unsigned long long ispan = hi - lo;
        const int64_t imin = (int64_t)(lo ^ kNbrSign), imax = (int64_t)(hi ^ kNbrSign), st = s.s[a];
        f.ilo[a] = lo ^ kNbrSign;
        f.olo[a] = 0, f.span[a] = 0, f.base[a] = 0;
        if (s.has_shape && (imin < 0 || imax >= s.in[a])) outside = true;
        if (ispan >= kNbrSpanLimit) overflow = true;
        if (outside || overflow) continue;
        const int64_t qmin = sc_floordiv(imin, st), rmin = imin - qmin * st;              // imin = qmin * st + rmin
        // outputs relative to qmin: the first one the smallest input can feed (through the last column), the last one the largest can
        int64_t lo_o = sc_floordiv(rmin + s.p[a] - (int64_t)(s.k[a] - 1) * s.d[a] + st - 1, st);
        int64_t hi_o = sc_floordiv(rmin + (int64_t)ispan + s.p[a], st);
        if (s.has_shape) {                                                                // (qmin is in [0, 2^31) here)
            lo_o = lo_o > -qmin ? lo_o : -qmin;
            hi_o = hi_o < s.out[a] - 1 - qmin ? hi_o : s.out[a] - 1 - qmin;
        }
        if (hi_o < lo_o) {
            empty = true;
            continue;
        }
        f.olo[a] = (unsigned long long)qmin + (unsigned long long)lo_o;
        f.span[a] = (unsigned long long)(hi_o - lo_o) + 1;
        f.base[a] = rmin + s.p[a] - lo_o * st;
    }
    f.ilo[3] = 0, f.span[3] = 1;
    if (has_batch) {
        unsigned long long lo, hi;
        nbr_axis(bounds, 3, lo, hi);
        f.ilo[3] = lo ^ kNbrSign;
        f.span[3] = hi - lo + 1;
        if (f.span[3] == 0) overflow = true;                                              // the whole int64 range
    }
    unsigned long long cells = 1;
    if (outside) overflow = false;                                                        // one verdict: the shape's
    if (empty || outside || overflow) cells = 0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        if (!cells) continue;
        if (f.span[a] > kNbrSpanLimit / cells) overflow = true, cells = 0;
        else cells *= f.span[a];
    }
    if (cells == 0)
#pragma unroll
        for (int a = 0; a < 3; a++) f.span[a] = 0;                                        // nothing is a candidate
    f.log2cap = nbr_log2cap(cells < (unsigned long long)vp ? cells : (unsigned long long)vp);
    f.refused = overflow || outside;
    *frame = f;
    if (overflow) counts[3] = 1;
    if (outside) counts[4] = 1;
}

__global__ __launch_bounds__(kNbrThreads) void k_sc_clear(const ScFrame *__restrict__ frame, int max_log2cap, ScSlot *__restrict__ slots)
{
    const int64_t cap = 1ll << (frame->log2cap < max_log2cap ? frame->log2cap : max_log2cap);
    for (int64_t i = (int64_t)blockIdx.x * kNbrThreads + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kNbrThreads)
        slots[i] = ScSlot{kNbrEmpty, ~0ull};
}

// the frame as the launches after k_sc_frame read it; the capacity is held inside the allocation whatever the words say (_emit trusts
// its caller to pass the workspace of _count: a wrong one must give wrong rows, not accesses outside it)
__device__ __forceinline__ ScFrame sc_load(const ScFrame *__restrict__ frame, int max_log2cap)
{
    ScFrame f = *frame;
    f.log2cap = f.log2cap < 6 ? 6 : f.log2cap > max_log2cap ? max_log2cap : f.log2cap;
    return f;
}

// candidate number -> (row, column); one 32-bit division where the number allows it
__device__ __forceinline__ void sc_split(int64_t c, uint32_t K, int64_t &v, uint32_t &k)
{
    if (((unsigned long long)c >> 32) == 0) {
        const uint32_t q = (uint32_t)c / K;
        v = q, k = (uint32_t)c - q * K;
    } else {
        v = c / K, k = (uint32_t)(c - v * K);
    }
}

// is (v, k) a candidate?  pos: the output's position in the box, key: its mixed-radix number (below 2^62)
__device__ __forceinline__ bool sc_candidate(const ScFrame &f, const ScShape &s, const int64_t *__restrict__ coords,
                                             const int64_t *__restrict__ batch, int64_t v, uint32_t k, unsigned long long pos[3],
                                             unsigned long long &key)
{
    int32_t ik[3];
    nbr_column(k, s.k, ik);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        // an input lies inside the measured box (below 2^62 from its start), base and the step are below 2^57: inside int64
        const int64_t t = f.base[a] + (int64_t)((unsigned long long)coords[v * 3 + a] - f.ilo[a]) - (int64_t)ik[a] * s.d[a];
        if (t < 0) return false;                                        // before the box (floor division: t = -1 is not output 0)
        unsigned long long q;
        if (((unsigned long long)t >> 32) == 0) {
            const uint32_t q32 = (uint32_t)t / (uint32_t)s.s[a];
            if (q32 * (uint32_t)s.s[a] != (uint32_t)t) return false;
            q = q32;
        } else {
            q = (unsigned long long)t / (unsigned long long)s.s[a];
            if (q * (unsigned long long)s.s[a] != (unsigned long long)t) return false;
        }
        if (q >= f.span[a]) return false;
        pos[a] = q;
    }
    const unsigned long long b = batch ? (unsigned long long)batch[v] - f.ilo[3] : 0ull;
    key = ((b * f.span[0] + pos[0]) * f.span[1] + pos[1]) * f.span[2] + pos[2];
    return true;
}

__global__ __launch_bounds__(kNbrThreads) void k_sc_insert(const int64_t *__restrict__ coords, const int64_t *__restrict__ batch, int64_t v,
                                                           ScShape s, const ScFrame *__restrict__ frame, int max_log2cap,
                                                           ScSlot *__restrict__ slots, int64_t *__restrict__ counts)
{
    const ScFrame f = sc_load(frame, max_log2cap);
    if (f.refused) return;
    const uint32_t K = (uint32_t)(s.k[0] * s.k[1] * s.k[2]);
    const int64_t n = v * (int64_t)K;
    unsigned long long entries = 0;
    // (every lane of a workgroup makes the same number of trips: the sum below runs on whole wavefronts)
    for (int64_t base = (int64_t)blockIdx.x * kNbrThreads; base < n; base += (int64_t)gridDim.x * kNbrThreads) {
        const int64_t c = base + threadIdx.x;
        if (c >= n) continue;
        int64_t vi;
        uint32_t k;
        sc_split(c, K, vi, k);
        unsigned long long pos[3], key;
        if (!sc_candidate(f, s, coords, batch, vi, k, pos, key)) continue;
        entries++;
        bool fresh;
        const int64_t h = nbr_claim(slots, key, f.log2cap, fresh);
        if (h >= 0) atomicMin(&slots[h].first, (unsigned long long)c);
    }
    const unsigned long long total = wave_sum_u64(entries);
    if (total && (threadIdx.x & (kWave - 1)) == 0) atomicAdd((unsigned long long *)&counts[1], total);
}

// the scan over the candidates (common.hpp): value = "c is the first candidate of its output"; apply numbers the outputs
struct ScNumber {
    static constexpr const char *kName = "k_sc_count_first", *kName2 = "k_sc_number";
    const int64_t *coords, *batch;
    ScShape s;
    const ScFrame *frame;
    int max_log2cap;
    ScSlot *slots;
    int64_t *out_coords, *out_batch;
    int64_t num_out;
    uint32_t K;

    __device__ int64_t first_slot(int64_t c, unsigned long long pos[3], int64_t &vi) const
    {
        const ScFrame f = sc_load(frame, max_log2cap);
        if (f.refused) return -1;
        uint32_t k;
        sc_split(c, K, vi, k);
        unsigned long long key;
        ScSlot sl;
        if (!sc_candidate(f, s, coords, batch, vi, k, pos, key)) return -1;
        const int64_t h = nbr_find(slots, key, f.log2cap, sl);
        return h >= 0 && sl.first == (unsigned long long)c ? h : -1;
    }
    __device__ unsigned long long value(int64_t c) const
    {
        unsigned long long pos[3];
        int64_t vi;
        return first_slot(c, pos, vi) >= 0;
    }
    // (the apply pass overwrites `first` of a slot with the output's row r while other lanes still read it.  Only the slot's first
    // candidate c_r writes, after its own read; any other candidate c of that output compares c with c_r or with r, and
    // c > c_r >= r -- rows are numbered in candidate order --, so it reads "not the first" either way)
    __device__ unsigned long long value2(int64_t c) const { return value(c); }
    __device__ void apply(int64_t c, unsigned long long mark, unsigned long long excl) const
    {
        if (!mark) return;
        unsigned long long pos[3];
        int64_t vi;
        const int64_t h = first_slot(c, pos, vi), row = (int64_t)excl;
        if (h < 0 || row >= num_out) return;
#pragma unroll
        for (int a = 0; a < 3; a++) out_coords[row * 3 + a] = (int64_t)(frame->olo[a] + pos[a]);
        if (out_batch) out_batch[row] = batch[vi];
        slots[h].first = (unsigned long long)row;
    }
};

__global__ __launch_bounds__(kNbrThreads) void k_sc_tables(const int64_t *__restrict__ coords, const int64_t *__restrict__ batch, int64_t v,
                                                           ScShape s, const ScFrame *__restrict__ frame, int max_log2cap,
                                                           const ScSlot *__restrict__ slots, int64_t num_out, int32_t *__restrict__ table_in,
                                                           int32_t *table_out, int64_t *__restrict__ counts)
{
    const ScFrame f = sc_load(frame, max_log2cap);
    if (f.refused) return;
    const uint32_t K = (uint32_t)(s.k[0] * s.k[1] * s.k[2]);
    const int64_t n = v * (int64_t)K;
    unsigned long long dups = 0;
    for (int64_t base = (int64_t)blockIdx.x * kNbrThreads; base < n; base += (int64_t)gridDim.x * kNbrThreads) {
        const int64_t c = base + threadIdx.x;
        if (c >= n) continue;
        int64_t vi;
        uint32_t k;
        sc_split(c, K, vi, k);
        unsigned long long pos[3], key;
        ScSlot sl;                                                      // (first: the output row by now)
        int32_t e = -1;
        if (sc_candidate(f, s, coords, batch, vi, k, pos, key) && nbr_find(slots, key, f.log2cap, sl) >= 0 && sl.first < (unsigned long long)num_out) {
            e = (int32_t)sl.first;
            dups += atomicCAS(&table_out[(int64_t)sl.first * K + k], -1, (int32_t)vi) != -1;
        }
        table_in[c] = e;
    }
    const unsigned long long total = wave_sum_u64(dups);
    if (total && (threadIdx.x & (kWave - 1)) == 0) atomicAdd((unsigned long long *)&counts[2], total);
}

// the arguments both entries share -> the shape, or a refusal
int sc_shape(int64_t v, const int32_t *ksz, const int32_t *stride, const int32_t *padding, const int32_t *dilation,
             const int64_t *spatial_shape, ScShape &s, int64_t &vp)
{
    if (v < 0 || !ksz || !stride || !padding || !dilation) return D3D_ERR_BAD_ARG;
    s.has_shape = spatial_shape != nullptr;
    for (int a = 0; a < 3; a++) {
        s.k[a] = ksz[a], s.s[a] = stride[a], s.p[a] = padding[a], s.d[a] = dilation[a];
        s.in[a] = s.out[a] = 0;
        if (s.k[a] < 1 || s.k[a] > 7 || s.s[a] < 1 || s.d[a] < 1 || s.p[a] < 0) return D3D_ERR_BAD_ARG;
    }
    for (int a = 0; a < 3; a++)
        if (s.s[a] > kScMaxStep || s.d[a] > kScMaxStep || s.p[a] > kScMaxStep) return D3D_ERR_UNSUPPORTED;
    for (int a = 0; a < 3 && spatial_shape; a++) {
        s.in[a] = spatial_shape[a];
        if (s.in[a] < 1) return D3D_ERR_BAD_ARG;
        if (s.in[a] > kScMaxShape) return D3D_ERR_UNSUPPORTED;
        const int64_t room = s.in[a] + 2 * (int64_t)s.p[a] - (int64_t)s.d[a] * (s.k[a] - 1) - 1;
        if (room < 0) return D3D_ERR_BAD_ARG;                           // dense conv3d has no output on this axis
        s.out[a] = room / s.s[a] + 1;
    }
    if (v > kRowMax) return D3D_ERR_UNSUPPORTED;
    const int64_t fan = sc_fanout(s);                                   // <= 343
    if (v > kRowMax / fan) return D3D_ERR_UNSUPPORTED;
    vp = v * fan;
    return D3D_OK;
}

}  // namespace

extern "C" size_t d3d_sparse_conv_map_workspace_bytes(int64_t v, const int32_t *kernel_size, const int32_t *stride, const int32_t *dilation)
{
    static const int32_t no_padding[3] = {0, 0, 0};
    ScShape s;
    int64_t vp = 0;
    if (sc_shape(std::max<int64_t>(v, 0), kernel_size, stride, no_padding, dilation, nullptr, s, vp) != D3D_OK) return 0;
    WsCarver w(nullptr, 0);
    sc_carve(w, vp, v * (int64_t)(s.k[0] * s.k[1] * s.k[2]));
    return w.off;
}

extern "C" int d3d_sparse_conv_map_count(const int64_t *coords, const int64_t *batch, int64_t v, const int32_t *kernel_size,
                                         const int32_t *stride, const int32_t *padding, const int32_t *dilation,
                                         const int64_t *spatial_shape, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    ScShape s;
    int64_t vp = 0;
    const int rc = sc_shape(v, kernel_size, stride, padding, dilation, spatial_shape, s, vp);
    if (rc != D3D_OK) return rc;
    if (!counts || (v > 0 && !coords)) return D3D_ERR_BAD_ARG;
    const int64_t K = s.k[0] * s.k[1] * s.k[2], n = v * K;
    WsCarver w(workspace, workspace_bytes);
    const ScWs ws = sc_carve(w, vp, n);
    if (v > 0 && (!workspace || !w.ok())) return D3D_ERR_WORKSPACE;
    D3D_HIP_CHECK(hipMemsetAsync(counts, 0, 5 * sizeof(int64_t), st));
    if (v == 0) return D3D_OK;
    D3D_HIP_CHECK(hipMemsetAsync(ws.bounds, 0, 8 * sizeof(unsigned long long), st));
    const int64_t vb = d3d_divup(v, kNbrThreads), nb = d3d_divup(n, kNbrThreads), tiles = d3d_divup(n, kScanTile);
    D3D_LAUNCH("k_vn_bounds", k_vn_bounds, dim3((unsigned)std::min<int64_t>(vb, kNbrBoundsBlocks)), dim3(kNbrThreads), 0, st, coords, batch, v,
               ws.bounds);
    D3D_LAUNCH("k_sc_frame", k_sc_frame, dim3(1), dim3(kWave), 0, st, ws.bounds, batch != nullptr, s, vp, ws.frame, counts);
    D3D_LAUNCH("k_sc_clear", k_sc_clear, dim3((unsigned)std::min<int64_t>(d3d_divup(1ll << ws.log2cap, kNbrThreads), kScClearBlocks)),
               dim3(kNbrThreads), 0, st, ws.frame, ws.log2cap, ws.slots);
    D3D_LAUNCH("k_sc_insert", k_sc_insert, dim3((unsigned)std::min(nb, kScBlocks)), dim3(kNbrThreads), 0, st, coords, batch, v, s, ws.frame,
               ws.log2cap, ws.slots, counts);
    const ScNumber f{coords, batch, s, ws.frame, ws.log2cap, ws.slots, nullptr, nullptr, 0, (uint32_t)K};
    D3D_LAUNCH(ScNumber::kName, k_scan_count<ScNumber>, dim3((unsigned)tiles), dim3(kScanBlock), 0, st, f, n, ws.bsum);
    D3D_LAUNCH("k_scan_bsum", k_scan_bsum, dim3(1), dim3(1024), 0, st, ws.bsum, tiles, counts, -1, 0, ~0ull, (int64_t *)nullptr,
               (const int64_t *)nullptr, 0);
    return D3D_OK;
}

extern "C" int d3d_sparse_conv_map_emit(const int64_t *coords, const int64_t *batch, int64_t v, const int32_t *kernel_size,
                                        const int32_t *stride, const int32_t *padding, const int32_t *dilation,
                                        const int64_t *spatial_shape, int64_t num_out, int64_t *out_coords, int64_t *out_batch,
                                        int32_t *table_in, int32_t *table_out, int64_t *counts, void *workspace, size_t workspace_bytes,
                                        void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    ScShape s;
    int64_t vp = 0;
    const int rc = sc_shape(v, kernel_size, stride, padding, dilation, spatial_shape, s, vp);
    if (rc != D3D_OK) return rc;
    if (!counts || num_out < 0 || num_out > vp || (v > 0 && (!coords || !table_in))) return D3D_ERR_BAD_ARG;
    if (num_out > 0 && (!out_coords || !table_out || (batch && !out_batch))) return D3D_ERR_BAD_ARG;
    const int64_t K = s.k[0] * s.k[1] * s.k[2], n = v * K;
    WsCarver w(workspace, workspace_bytes);
    const ScWs ws = sc_carve(w, vp, n);
    if (v > 0 && (!workspace || !w.ok())) return D3D_ERR_WORKSPACE;
    if (v == 0) return D3D_OK;
    if (num_out > 0) D3D_HIP_CHECK(hipMemsetAsync(table_out, 0xff, (size_t)num_out * K * sizeof(int32_t), st));
    const int64_t nb = d3d_divup(n, kNbrThreads), tiles = d3d_divup(n, kScanTile);
    const ScNumber f{coords, batch, s, ws.frame, ws.log2cap, ws.slots, out_coords, batch ? out_batch : nullptr, num_out, (uint32_t)K};
    D3D_LAUNCH(ScNumber::kName2, k_scan_apply<ScNumber>, dim3((unsigned)tiles), dim3(kScanBlock), 0, st, f, n, ws.bsum);
    D3D_LAUNCH("k_sc_tables", k_sc_tables, dim3((unsigned)std::min(nb, kScBlocks)), dim3(kNbrThreads), 0, st, coords, batch, v, s, ws.frame,
               ws.log2cap, ws.slots, num_out, table_in, table_out, counts);
    return D3D_OK;
}
