// boxpair.hip -- the PAIRED box operators on MI355X (gfx950): IoU / GIoU / DIoU of box i of one set against box i of the other,
// and the "3D IoU" (BEV IoU x z-interval IoU) of such pairs, each with the pair's partial derivatives on request.  An
// extension: the reference offers the [N,M] matrices only (d3d/box/iou.h:7-69), and a detector's regression loss wants the
// diagonal -- prediction i against its assigned target i.
//
// One pair per lane, 256 lanes per workgroup, nothing shared between lanes: a lane loads its two rows (widening them where the
// arithmetic is wider than the memory), builds both geometries and runs the SAME per-pair functions of geom.hpp the matrix
// kernels run, so a pair's value is the value the matrix holds on its diagonal.  With `jac` the lane also stores the pair's
// 5 + 5 (7 + 7) partial derivatives, one contiguous row: every pair owns its gradient rows, so the backward pass is
// grad[i] * jac[i, :] -- no atomics, no workspace, no kernel in the backward pass at all.
#include "common.hpp"
#include "geom.hpp"

namespace {

constexpr int kPairLanes = 256;
enum { kPairBox = 0, kPairRbox = 1, kPairGiou = 2, kPairDiou = 3 };

template <typename T, int K> __device__ __forceinline__ void store_jac(T *row, const T (&ga)[K], const T (&gb)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++) { row[k] = ga[k]; row[K + k] = gb[k]; }
}

// ---------------------------------------------------------------- 2-D: box / rbox / grbox / drbox
// TIn: the boxes and `ious` in memory; T: the arithmetic and `jac`.
template <typename TIn, typename T, int KIND, bool GRAD>
__global__ __launch_bounds__(kPairLanes) void k_iou_paired(const TIn *__restrict__ b1, const TIn *__restrict__ b2, int64_t n,
                                                           TIn *__restrict__ ious, T *__restrict__ jac)
{
    const int64_t i = (int64_t)blockIdx.x * kPairLanes + threadIdx.x;
    if (i >= n) return;
    T ra[5], rb[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { ra[k] = (T)b1[i * 5 + k]; rb[k] = (T)b2[i * 5 + k]; }
    const BoxGeom<T> a = make_geom<T>(ra[0], ra[1], ra[2], ra[3], ra[4]), b = make_geom<T>(rb[0], rb[1], rb[2], rb[3], rb[4]);
    T v = 0, ga[5] = {0, 0, 0, 0, 0}, gb[5] = {0, 0, 0, 0, 0};
    if constexpr (KIND == kPairBox || KIND == kPairRbox) {
        constexpr bool ROTATED = KIND == kPairRbox;
        // the candidate test and the per-pair function of k_iou_small / k_iou_grad_small (box.hip)
        if (aabb_gap(cand_aabb(a, ROTATED), cand_aabb(b, ROTATED)) > 0.f) {
            if constexpr (!GRAD) v = ROTATED ? iou_rbox(a, b) : iou_aabb(a, b);
            else if constexpr (ROTATED) v = iou_rbox_grad<T>(a, b, ra[2], ra[3], rb[2], rb[3], ga, gb);
            else v = iou_aabb_grad<T, T>(a, b, ra, rb, ga, gb);
        }
    } else {
        constexpr int LOSS = KIND == kPairGiou ? 0 : 1;
        // the rule of geom.hpp (loss_rbox_apart): the forward-only form where it applies, the complete routine for the pairs it
        // defers -- as k_loss_iou does, so the value is the matrix's.  With GRAD the derivatives of EVERY pair come from the
        // complete routine (what k_loss_iou_grad runs); its own return value is not used: it recovers the intersection from the
        // IoU and would differ from the forward's by rounding, and a pair's value must not depend on who asks for a gradient.
        // The price: a deferred pair's clip (~500 of the complete routine's ~3000 instructions) runs in both.
        const HullPre<T> ha = hull_pre<T>(a), hb = hull_pre<T>(b);
        bool defer;
        v = loss_rbox_apart<T, LOSS>(a, ha, b, hb, defer);
        if (__any(defer)) {
            const T full = loss_complete<T, LOSS>(a, b);
            v = defer ? full : v;
        }
        if constexpr (GRAD) loss_iou_rbox<T, LOSS, true>(a, b, ra[2], ra[3], rb[2], rb[3], ga, gb);
    }
    ious[i] = (TIn)v;
    if constexpr (GRAD) store_jac<T, 5>(jac + i * 10, ga, gb);
}

// ---------------------------------------------------------------- 3-D: BEV IoU x z-interval IoU
// rows (x, y, z, lx, ly, lz, rz); the definition of load3d / k_iou3d_small (box.hip; reference d3d/dgal_wrap.h:45-91):
// bev(x, y, lx, ly, rz) * max(min(zmax) - max(zmin), 0) / max(max(zmax) - min(zmin), 1e-6), 0 where the BEV IoU is 0.
// Derivatives: d / d (x, y, lx, ly, rz) = zfactor * d bev;  d / d z, d / d lz = bev * d zfactor, and zfactor = zi / zu moves with
// the FOUR interval ends the min / max select (zmax = z + lz / 2, zmin = z - lz / 2) -- selects, not branches.  On a tie either
// box may be named (a kink: any one-sided derivative).  zi == 0 (ranges apart or only touching): value and row are 0; the floor
// of zu active: zu does not move.
template <typename TIn, typename T, bool ROTATED, bool GRAD>
__global__ __launch_bounds__(kPairLanes) void k_iou3d_paired(const TIn *__restrict__ b1, const TIn *__restrict__ b2, int64_t n,
                                                             TIn *__restrict__ ious, T *__restrict__ jac)
{
    const int64_t i = (int64_t)blockIdx.x * kPairLanes + threadIdx.x;
    if (i >= n) return;
    T ra[7], rb[7];
#pragma unroll
    for (int k = 0; k < 7; k++) { ra[k] = (T)b1[i * 7 + k]; rb[k] = (T)b2[i * 7 + k]; }
    const BoxGeom<T> a = make_geom<T>(ra[0], ra[1], ra[3], ra[4], ra[6]), b = make_geom<T>(rb[0], rb[1], rb[3], rb[4], rb[6]);
    const T azmax = ra[2] + ra[5] / 2, azmin = ra[2] - ra[5] / 2, bzmax = rb[2] + rb[5] / 2, bzmin = rb[2] - rb[5] / 2;
    T bev = 0, ga[5] = {0, 0, 0, 0, 0}, gb[5] = {0, 0, 0, 0, 0};
    if (aabb_gap(cand_aabb(a, ROTATED), cand_aabb(b, ROTATED)) > 0.f) {
        if constexpr (!GRAD) bev = ROTATED ? iou_rbox(a, b) : iou_aabb(a, b);
        else if constexpr (ROTATED) bev = iou_rbox_grad<T>(a, b, ra[3], ra[4], rb[3], rb[4], ga, gb);
        else {
            const T qa[5] = {ra[0], ra[1], ra[3], ra[4], ra[6]}, qb[5] = {rb[0], rb[1], rb[3], rb[4], rb[6]};
            bev = iou_aabb_grad<T, T>(a, b, qa, qb, ga, gb);
        }
    }
    const T imax = fmin(azmax, bzmax), imin = fmax(azmin, bzmin), umax = fmax(azmax, bzmax), umin = fmin(azmin, bzmin);
    const T zi = fmax(imax - imin, (T)0), zu = fmax(umax - umin, (T)1e-6);
    T v = 0;
    if (bev != 0) v = bev * (zi / zu);
    ious[i] = (TIn)v;
    if constexpr (GRAD) {
        const bool live = (bev != 0) & (imax - imin > 0);
        // a's end is the inner one (then b's is the outer one) at the top / at the bottom
        const bool atop = azmax < bzmax, abot = azmin > bzmin;
        const T zf = zi / zu, izu = (T)1 / zu, moves = (umax - umin > (T)1e-6) ? (T)1 : (T)0, out = zf * moves;
        // d zfactor / d (zmax, zmin) of a and of b:  (d zi - zfactor d zu) / zu
        const T atopd = ((atop ? (T)1 : (T)0) - (atop ? (T)0 : out)) * izu, abotd = ((abot ? (T)0 : out) - (abot ? (T)1 : (T)0)) * izu;
        const T btopd = ((atop ? (T)0 : (T)1) - (atop ? out : (T)0)) * izu, bbotd = ((abot ? out : (T)0) - (abot ? (T)0 : (T)1)) * izu;
        const T s = live ? zf : (T)0, t = live ? bev : (T)0;
        const T ja[7] = {s * ga[0], s * ga[1], t * (atopd + abotd), s * ga[2], s * ga[3], t * ((atopd - abotd) / 2), s * ga[4]};
        const T jb[7] = {s * gb[0], s * gb[1], t * (btopd + bbotd), s * gb[2], s * gb[3], t * ((btopd - bbotd) / 2), s * gb[4]};
        store_jac<T, 7>(jac + i * 14, ja, jb);
    }
}

// the checks the two entries share, in the header's order; *launch = there is something to do
int paired_check(const void *b1, const void *b2, int64_t n, int32_t dtype, const void *ious, bool *launch)
{
    *launch = false;
    if (n < 0) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64 && dtype != D3D_F32_WIDE) return D3D_ERR_UNSUPPORTED;
    if (n == 0) return D3D_OK;
    if (!b1 || !b2 || !ious || d3d_divup(n, kPairLanes) > 0x7fffffffll) return D3D_ERR_BAD_ARG;
    *launch = true;
    return D3D_OK;
}

}  // namespace

extern "C" int d3d_iou2d_paired(const void *boxes1, const void *boxes2, int64_t n, int32_t iou_type, int32_t dtype, void *ious,
                                void *jac, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (n < 0) return D3D_ERR_BAD_ARG;
    if (iou_type != D3D_IOU_BOX && iou_type != D3D_IOU_RBOX && iou_type != D3D_IOU_GRBOX && iou_type != D3D_IOU_DRBOX) return D3D_ERR_UNSUPPORTED;
    bool launch;
    if (const int rc = paired_check(boxes1, boxes2, n, dtype, ious, &launch); rc != D3D_OK || !launch) return rc;
    const dim3 grid((unsigned)d3d_divup(n, kPairLanes));
    return dispatch_dtype<D3D_F32, D3D_F64, D3D_F32_WIDE>(dtype, [&](auto p) {
        typedef typename decltype(p)::T T;
        typedef typename decltype(p)::B B;
        return dispatch_int<D3D_IOU_BOX, D3D_IOU_RBOX, D3D_IOU_GRBOX, D3D_IOU_DRBOX>(iou_type, [&](auto t) {
            constexpr int V = decltype(t)::value, KIND = V == D3D_IOU_BOX ? kPairBox : V == D3D_IOU_RBOX ? kPairRbox : V == D3D_IOU_GRBOX ? kPairGiou : kPairDiou;
            return dispatch(jac != nullptr, [&](auto g) {
                D3D_LAUNCH(g ? "k_iou_paired<grad>" : "k_iou_paired", (k_iou_paired<B, T, KIND, g>), grid, dim3(kPairLanes), 0, st,
                           (const B *)boxes1, (const B *)boxes2, n, (B *)ious, (T *)jac);
                return D3D_OK;
            });
        });
    });
}

extern "C" int d3d_iou3d_paired(const void *boxes1, const void *boxes2, int64_t n, int32_t rotated, int32_t dtype, void *ious,
                                void *jac, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    bool launch;
    if (const int rc = paired_check(boxes1, boxes2, n, dtype, ious, &launch); rc != D3D_OK || !launch) return rc;
    const dim3 grid((unsigned)d3d_divup(n, kPairLanes));
    return dispatch_dtype<D3D_F32, D3D_F64, D3D_F32_WIDE>(dtype, [&](auto p) {
        typedef typename decltype(p)::T T;
        typedef typename decltype(p)::B B;
        return dispatch(rotated != 0, [&](auto r) {
            return dispatch(jac != nullptr, [&](auto g) {
                D3D_LAUNCH(g ? "k_iou3d_paired<grad>" : "k_iou3d_paired", (k_iou3d_paired<B, T, r, g>), grid, dim3(kPairLanes), 0, st,
                           (const B *)boxes1, (const B *)boxes2, n, (B *)ious, (T *)jac);
                return D3D_OK;
            });
        });
    });
}
