// camera.hip -- TransformSet.transform_points and TransformSet.project_points_to_camera of the reference
// (d3d/abstraction.pyx:971-977, 979-1035): a cloud through an extrinsic and a camera matrix, the optional 5-coefficient lens
// distortion, the image coordinates and the ascending indices of the points in view (mask) and in front of the camera (dmask).
// The reference runs it in numpy on one core with about ten temporaries of N elements; here it is one streaming pass per
// launch, fp64 arithmetic on fp32 / fp64 rows read in place, no contraction (-ffp-contract=off).
//
// The compaction keeps point order, so it needs a prefix sum over the cloud.  Three launches, none of which waits on another
// workgroup: k_cam_count (flags per point, one packed count per workgroup and camera), k_scan_tile_sums (one workgroup per camera
// scans those counts and leaves K and Kd), k_cam_emit (the same flags again -- the same expressions give the same bits --
// a scan inside the workgroup, the stores).  The flags are recomputed instead of stored: 12-16 bytes read again per point
// against 16 bytes of uv per point and camera that a stored form would have to keep for the gather.
// Up to kCamMax camera records travel by value in the kernel arguments (scalar loads, wavefront-uniform): the cloud is read
// once per launch for all of them.
#include "common.hpp"

namespace {

constexpr int kCamMax = 8;                      // records per launch (8 x 256 bytes of kernel arguments); more: further launches
constexpr int kCamThreads = 256, kCamItems = 4, kCamTile = kCamThreads * kCamItems;
constexpr double kPreMask = 20.0;               // the tolerance of the mask ahead of the distortion, in pixels (abstraction.pyx:1005)

struct CamSet { D3DCamera cam[kCamMax]; };
struct Rt34 { double m[12]; };

// (x, y, z) of row i, widened.  VEC: rows of four elements on a 16-byte boundary -- fp32: one 16-byte load per lane; fp64: a
// 16-byte load and an 8-byte one.  Any other row length: three element loads (rows of 3 floats are 12 bytes apart, no wider
// load is aligned; consecutive lanes still use every byte of the lines they touch).
template <class T>
__device__ __forceinline__ void load_xyz(const T *__restrict__ points, int64_t i, int stride, bool vec, double &x, double &y, double &z)
{
    const T *p = points + i * stride;
    if (vec) {
        if constexpr (sizeof(T) == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(p);
            x = (double)q.x; y = (double)q.y; z = (double)q.z;
        } else {
            const double2 q = *reinterpret_cast<const double2 *>(p);
            x = q.x; y = q.y; z = (double)p[2];
        }
    } else {
        x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    }
}

// out = R . p + t, each component summed left to right (abstraction.pyx:976, 991-994)
__device__ __forceinline__ void apply_rt(const double *rt, double x, double y, double z, double &X, double &Y, double &Z)
{
    X = rt[0] * x + rt[1] * y + rt[2] * z + rt[3];
    Y = rt[4] * x + rt[5] * y + rt[6] * z + rt[7];
    Z = rt[8] * x + rt[9] * y + rt[10] * z + rt[11];
}

constexpr unsigned long long kInView = 1ull << 32, kInFront = 1ull;      // the packed pair of a point: (mask : 32 | dmask : 32)

// abstraction.pyx:994-1024 for one point and one camera; returns the packed flags
__device__ __forceinline__ unsigned long long project(const D3DCamera &c, double x, double y, double z, double &u, double &v)
{
    double X, Y, Z;
    apply_rt(c.rt, x, y, z, X, Y, Z);
    const double h0 = c.P[0] * X + c.P[1] * Y + c.P[2] * Z;
    const double h1 = c.P[3] * X + c.P[4] * Y + c.P[5] * Z;
    const double d = c.P[6] * X + c.P[7] * Y + c.P[8] * Z;
    u = h0 / d;                                   // IEEE divisions: d = 0, NaN and inf as numpy has them (:996)
    v = h1 / d;
    const bool front = d > 0;                     // :999
    const double W = (double)c.width, H = (double)c.height;
    bool view;
    if (c.has_dist) {
        const bool pre = -kPreMask < u && u < W + kPreMask && -kPreMask < v && v < H + kPreMask;      // :1006-1007, no d here
        const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3], k3 = c.dist[4];
        u = (u - c.cx) / c.fx;                    // :1013
        v = (v - c.cy) / c.fy;
        const double r2 = u * u + v * v;
        const double auv = 2 * u * v, au = r2 + 2 * u * u, av = r2 + 2 * v * v;
        const double cd = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
        const double ud = u * cd + p1 * auv + p2 * au;
        const double vd = v * cd + p1 * av + p2 * auv;
        u = ud * c.fx + c.cx;                     // :1020
        v = vd * c.fy + c.cy;
        view = pre && 0 < u && u < W && 0 < v && v < H && front;                                       // :1023-1024
    } else {
        view = 0 < u && u < W && 0 < v && v < H && front;                                              // :1000
    }
    return (view ? kInView : 0ull) | (front ? kInFront : 0ull);
}

// bsum[c * nb + workgroup] = (points in view : 32 | points in front : 32) of the workgroup's tile for camera c.  (Not
// tile_sum_u64: with a slot per camera ONE barrier serves up to eight cameras.)
template <class T>
__global__ __launch_bounds__(kCamThreads) void k_cam_count(const T *__restrict__ points, int64_t n, int stride, int vec, CamSet cs,
                                                           int ncam, unsigned long long *__restrict__ bsum, int64_t nb)
{
    __shared__ unsigned long long sm[kCamMax][kCamThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const int64_t base = tile_item<kCamThreads, kCamItems>(blockIdx.x);
    double x[kCamItems], y[kCamItems], z[kCamItems];
#pragma unroll
    for (int k = 0; k < kCamItems; k++) {
        const int64_t i = base + (int64_t)k * kWave;
        x[k] = y[k] = z[k] = 0.0;
        if (i < n) load_xyz(points, i, stride, vec != 0, x[k], y[k], z[k]);
    }
    for (int c = 0; c < ncam; c++) {
        unsigned long long s = 0;
#pragma unroll
        for (int k = 0; k < kCamItems; k++) {
            double u, v;
            if (base + (int64_t)k * kWave < n) s += project(cs.cam[c], x[k], y[k], z[k], u, v);
        }
        s = wave_sum_u64(s);
        if (lane == 0) sm[c][w] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < ncam) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < kCamThreads / kWave; k++) t += sm[threadIdx.x][k];
        bsum[(int64_t)threadIdx.x * nb + blockIdx.x] = t;
    }
}

// Camera c writes into its own section of the outputs: uv + c * n * 2, mask + c * n, dmask + c * n.  ALL_UV: uv row i = point
// i; else uv row j = the j-th point in view.  dmask may be NULL.
template <class T, bool ALL_UV>
__global__ __launch_bounds__(kCamThreads) void k_cam_emit(const T *__restrict__ points, int64_t n, int stride, int vec, CamSet cs,
                                                          int ncam, const unsigned long long *__restrict__ bsum_excl, int64_t nb,
                                                          double *__restrict__ uv, int64_t *__restrict__ mask, int64_t *__restrict__ dmask)
{
    __shared__ unsigned long long sm[kCamMax][kCamThreads / kWave];
    const int64_t base = tile_item<kCamThreads, kCamItems>(blockIdx.x);
    double x[kCamItems], y[kCamItems], z[kCamItems];
#pragma unroll
    for (int k = 0; k < kCamItems; k++) {
        const int64_t i = base + (int64_t)k * kWave;
        x[k] = y[k] = z[k] = 0.0;
        if (i < n) load_xyz(points, i, stride, vec != 0, x[k], y[k], z[k]);
    }
    for (int c = 0; c < ncam; c++) {
        double u[kCamItems], v[kCamItems];
        unsigned long long f[kCamItems], ex[kCamItems], total;
#pragma unroll
        for (int k = 0; k < kCamItems; k++) {
            f[k] = 0;
            u[k] = v[k] = 0.0;
            if (base + (int64_t)k * kWave < n) f[k] = project(cs.cam[c], x[k], y[k], z[k], u[k], v[k]);
        }
        tile_excl_scan_u64<kCamThreads, kCamItems>(f, ex, sm[c], &total);      // (a slot per camera: its one barrier is enough)
        const unsigned long long before = bsum_excl[(int64_t)c * nb + blockIdx.x];
        double2 *uvc = reinterpret_cast<double2 *>(uv) + (int64_t)c * n;
#pragma unroll
        for (int k = 0; k < kCamItems; k++) {
            const int64_t i = base + (int64_t)k * kWave;
            if (i >= n) continue;
            const unsigned long long off = before + ex[k];   // (both fields < n: the sections hold n rows)
            if (ALL_UV) uvc[i] = make_double2(u[k], v[k]);
            if (f[k] & kInView) {
                mask[(int64_t)c * n + (int64_t)(off >> 32)] = i;
                if (!ALL_UV) uvc[(int64_t)(off >> 32)] = make_double2(u[k], v[k]);
            }
            if (dmask && (f[k] & kInFront)) dmask[(int64_t)c * n + (int64_t)(off & 0xffffffffull)] = i;
        }
    }
}

// one thread per element of out[n, stride]: columns 0..2 = R . p + t, the others widened
template <class T>
__global__ __launch_bounds__(256) void k_transform_points(const T *__restrict__ points, int64_t n, int stride, Rt34 rt,
                                                          double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * stride) return;
    const int64_t i = e / stride;
    const int j = (int)(e - i * stride);
    if (j >= 3) {
        out[e] = (double)points[e];
        return;
    }
    const T *p = points + i * stride;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    out[e] = rt.m[4 * j] * x + rt.m[4 * j + 1] * y + rt.m[4 * j + 2] * z + rt.m[4 * j + 3];
}

}  // namespace

extern "C" size_t d3d_project_points_workspace_bytes(int64_t n, int32_t ncam)
{
    if (n < 0 || ncam < 1) return 0;
    return d3d_align_up((size_t)ncam * (size_t)d3d_divup(n, kCamTile) * sizeof(unsigned long long)) + 256;
}

// TransformSet.project_points_to_camera (reference d3d/abstraction.pyx:979-1035) for ncam cameras over one cloud.
extern "C" int d3d_project_points(const void *points, int64_t n, int32_t stride, int32_t dtype, const D3DCamera *cameras, int32_t ncam,
                                  uint32_t flags, double *uv, int64_t *mask, int64_t *dmask, int64_t *counts, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n > 0x7fffffffll || stride < 3 || ncam < 1 || !cameras || !counts) return D3D_ERR_BAD_ARG;
    if (flags & ~(uint32_t)(D3D_PROJECT_ALL_UV | D3D_PROJECT_DMASK)) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64) return D3D_ERR_BAD_ARG;
    const bool want_d = (flags & D3D_PROJECT_DMASK) != 0;
    if (n > 0 && (!points || !uv || !mask || (want_d && !dmask))) return D3D_ERR_BAD_ARG;
    const int64_t nb = d3d_divup(n, kCamTile);
    if (nb > 0 && (!workspace || workspace_bytes < d3d_project_points_workspace_bytes(n, ncam))) return D3D_ERR_WORKSPACE;
    unsigned long long *bsum = (unsigned long long *)workspace;
    const int vec = stride == 4 && ((uintptr_t)points & 15) == 0;
    for (int32_t c0 = 0; c0 < ncam; c0 += kCamMax) {
        const int nc = ncam - c0 < kCamMax ? ncam - c0 : kCamMax;
        CamSet cs;
        for (int c = 0; c < kCamMax; c++) cs.cam[c] = cameras[c0 + (c < nc ? c : 0)];
        unsigned long long *bs = bsum + (int64_t)c0 * nb;
        double *uvc = uv + (int64_t)c0 * n * 2;
        int64_t *mc = mask + (int64_t)c0 * n, *dc = want_d ? dmask + (int64_t)c0 * n : nullptr;
        const int rc = dispatch_dtype<D3D_F32, D3D_F64>(dtype, [&](auto p) -> int {
            typedef typename decltype(p)::T T;
            if (nb > 0)
                D3D_LAUNCH("k_cam_count", k_cam_count<T>, dim3((unsigned)nb), dim3(kCamThreads), 0, st, (const T *)points, n, (int)stride, vec,
                           cs, nc, bs, nb);
            D3D_LAUNCH("k_scan_tile_sums", k_scan_tile_sums<kSumsPacked>, dim3((unsigned)nc), dim3(1024), 0, st, bs, nb, counts + 2 * c0);
            if (nb == 0) return D3D_OK;
            return dispatch((flags & D3D_PROJECT_ALL_UV) != 0, [&](auto all) -> int {
                D3D_LAUNCH("k_cam_emit", (k_cam_emit<T, all>), dim3((unsigned)nb), dim3(kCamThreads), 0, st, (const T *)points, n, (int)stride,
                           vec, cs, nc, bs, nb, uvc, mc, dc);
                return D3D_OK;
            });
        });
        if (rc != D3D_OK) return rc;
    }
    return D3D_OK;
}

// TransformSet.transform_points (reference d3d/abstraction.pyx:971-977): out[n, stride] f64.
extern "C" int d3d_transform_points(const void *points, int64_t n, int32_t stride, int32_t dtype, const double *rt, double *out,
                                    void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || stride < 3 || !rt) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64) return D3D_ERR_BAD_ARG;
    if (n == 0) return D3D_OK;
    if (!points || !out) return D3D_ERR_BAD_ARG;
    Rt34 m;
    for (int k = 0; k < 12; k++) m.m[k] = rt[k];
    const int64_t blocks = d3d_divup(n * stride, 256);
    if (blocks > 0x7fffffffll) return D3D_ERR_BAD_ARG;
    return dispatch_dtype<D3D_F32, D3D_F64>(dtype, [&](auto p) -> int {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH("k_transform_points", k_transform_points<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T *)points, n, (int)stride, m,
                   out);
        return D3D_OK;
    });
}
