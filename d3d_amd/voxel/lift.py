"""d3d_amd.voxel.lift -- camera features into the ego grid: the "lift, splat" view transform of LSS / BEVDet / BEVDepth / BEVFusion
(bev_pool).  Every pixel of every camera carries a depth distribution over D bins and a context row of C channels; the frustum points
are placed in the grid once per set of calibrations (FrustumMap) and every cell gets the sum of depth[p] * feat[pixel(p)] over its
points (lift_splat), as voxel rows [V, C] with coords -- what the sparse convolutions take as they are and voxel_to_bev turns into the
BEV map.  An extension (the reference stops at projecting points into the cameras).

    pre, post = frustum_matrices(rots, trans, intrins, post_rots, post_trans)        # host, fp64, rounded once to fp32
    fmap = FrustumMap(us, vs, ds, pre, post, bounds, shape, cams_per_sample=6)        # once per frame; forward and backward reuse it
    rows = lift_splat(depth, feat, fmap)                                              # [V, C]; depth [S, D, H, W], feat [S, H, W, C]
    bev  = lift_splat_bev(depth, feat, fmap)                                          # [B, C * Z, Y, X]

The [S * D * H * W, C] product never exists.  No float atomics: the map is inverted once (VoxelIndex) and a cell's points are folded
strictly in ascending point number, so the results are the same bits on every run (kernels and the exact rules: csrc/vlift.hip,
include/d3d_hip.h).  The geometry gets NO gradient.

Out of scope: deriving (pre, post) from a TransformSet.
"""
import ctypes

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._rows import FEATURE_CODES, ROW_MAX, as_tensor, back_to_caller, check_owner_device, device_of, dtype_code, to_owner
from ._coords import _triple
from .dense import VoxelDenseMap, voxel_to_bev
from .pool import VoxelIndex


def _host_f32(x, what, shape):
    """x (tensor anywhere or numpy, any float dtype) -> a contiguous float32 numpy array of `shape` (-1: any); one rounding"""
    x, _ = as_tensor(x, what)
    if not x.dtype.is_floating_point:
        raise ValueError("%s must be a floating-point array, not %s" % (what, x.dtype))
    if x.dim() != len(shape) or any(want not in (-1, have) for want, have in zip(shape, x.shape)):
        raise ValueError("%s must have the shape %s, not %r" % (what, list(shape), tuple(x.shape)))
    return np.ascontiguousarray(x.detach().cpu().to(torch.float32).numpy())


def grid_of(bounds, shape):
    """(bounds, shape) -> (lo [3] float32, size [3] float32, shape (n0, n1, n2)): bounds = (xmin, xmax, ymin, ymax, zmin, zmax) as the
    voxelizer's, lo = the minima, size = (max - min) / shape in fp64, each rounded once to fp32.  ValueError for a shape below 1 and a
    size that is not positive and finite.  Nothing here needs a GPU"""
    shape = _triple(shape.tolist() if isinstance(shape, np.ndarray) else shape, "shape")
    if any(n < 1 for n in shape):
        raise ValueError("shape must be >= 1 per axis, not %r" % (shape,))
    b = np.asarray(bounds, np.float64).reshape(-1)
    if b.shape != (6,):
        raise ValueError("bounds must be six numbers (xmin, xmax, ymin, ymax, zmin, zmax)")
    lo = b[0::2].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        size = ((b[1::2] - b[0::2]) / np.asarray(shape, np.float64)).astype(np.float32)
    if not np.all(np.isfinite(size) & (size > 0)):
        raise ValueError("bounds must give a positive, finite cell size per axis, not %r" % (size.tolist(),))
    return lo, size, shape


class FrustumMap:
    """Where every frustum point of one set of calibrations lands in the ego grid.

    :param us, vs, ds: [W], [H], [D] the frustum's pixel columns, pixel rows and depth bins (given explicitly: no linspace rounding
        is part of the contract); float, used as float32
    :param pre, post: [S, 3, 4] the two affine maps of S = B * cams_per_sample cameras (frustum_matrices makes them); float32
    :param bounds: (xmin, xmax, ymin, ymax, zmin, zmax) of the grid, as the voxelizer's
    :param shape: (n0, n1, n2) cells per coordinate column (x, y, z)
    :param cams_per_sample: N; camera s belongs to sample s // N
    Tensors (GPU or host) or numpy arrays, as everywhere in this layer.

    Point p = ((s * D + d) * H + h) * W + w; in fp32, one rounding per operation: a = (us[w], vs[h], ds[d]), q = pre[s] (a, 1),
    e = (q0 * q2, q1 * q2, q2), x = post[s] (e, 1), t = (x - lo) / size; the point is a member iff 0 <= t < shape on every axis and
    lands in cell (int) t.  Points with t in (-1, 0) are NOT members (LSS's .long() would fold them into cell 0).

    Holds, on the GPU: `mapping` [K] int64 (the row of every point, -1 for none), `coords` [V, 3] int64 (x, y, z) and `batch_index`
    [V] int64, rows numbered by ascending (sample, x, y, z); `index`, the VoxelIndex of the mapping (mapping kept); and `num_voxels`,
    `num_points` = K, `num_members`, `num_cameras` = S, `batch_size` = B, `cams_per_sample`, `frustum` = (D, H, W), `shape`, `lo`,
    `size`, `device`.  Building it reads two numbers back once (and the index two more).  Nothing here is differentiable."""

    def __init__(self, us, vs, ds, pre, post, bounds, shape, cams_per_sample):
        given = (pre, post, us, vs, ds)
        us, vs, ds = _host_f32(us, "us", (-1,)), _host_f32(vs, "vs", (-1,)), _host_f32(ds, "ds", (-1,))
        pre, post = _host_f32(pre, "pre", (-1, 3, 4)), _host_f32(post, "post", (-1, 3, 4))
        lo, size, shape = grid_of(bounds, shape)
        if isinstance(cams_per_sample, bool) or not isinstance(cams_per_sample, (int, np.integer)) or cams_per_sample < 1:
            raise ValueError("cams_per_sample must be an int >= 1, not %r" % (cams_per_sample,))
        n, s = int(cams_per_sample), pre.shape[0]
        if post.shape[0] != s:
            raise ValueError("pre holds %d cameras, post %d" % (s, post.shape[0]))
        if s % n:
            raise ValueError("%d cameras are no multiple of cams_per_sample = %d" % (s, n))
        w, h, d = len(us), len(vs), len(ds)
        k, b = s * d * h * w, s // n
        cells = b * shape[0] * shape[1] * shape[2]
        if k > ROW_MAX or cells > ROW_MAX:
            raise ValueError("FrustumMap takes at most 2^31 - 1 frustum points and grid cells (batch x shape)")
        dev = device_of(*given)                              # (every refusal above comes before a GPU is needed)
        self.device, self.num_points, self.num_cameras, self.batch_size, self.cams_per_sample = dev, k, s, b, n
        self.frustum, self.shape, self.lo, self.size = (d, h, w), shape, lo, size
        self._dense = {}
        with torch.cuda.device(dev):
            lib = _lib.load()
            g_us, g_vs, g_ds, g_pre, g_post = _lib.ship(dev, us, vs, ds, pre, post)
            c_shape = (ctypes.c_int32 * 3)(*shape)
            counts = torch.empty((2,), dtype=torch.int64, device=dev)
            ws = _lib.workspace(lib.d3d_frustum_map_workspace_bytes(k, cells), dev)
            rc = lib.d3d_frustum_map_count(_lib.ptr(g_us), w, _lib.ptr(g_vs), h, _lib.ptr(g_ds), d, _lib.ptr(g_pre), _lib.ptr(g_post), s, n,
                                           lo.ctypes.data_as(ctypes.c_void_p), size.ctypes.data_as(ctypes.c_void_p), c_shape,
                                           _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            _lib.check(rc, "frustum_map")
            v, members = counts.tolist()                     # the one read-back of a frame's map
            self.mapping = torch.empty((k,), dtype=torch.int64, device=dev)
            self.coords = torch.empty((v, 3), dtype=torch.int64, device=dev)
            self.batch_index = torch.empty((v,), dtype=torch.int64, device=dev)
            rc = lib.d3d_frustum_map_emit(w, h, d, s, n, c_shape, v, _lib.ptr(self.mapping), _lib.ptr(self.coords),
                                          _lib.ptr(self.batch_index), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            _lib.check(rc, "frustum_map")
            self.num_voxels, self.num_members = v, members
            self.index = VoxelIndex(self.mapping, v)
            self.mapping = self.index.mapping

    def dense_map(self, axes=(2, 1, 0)):
        """the VoxelDenseMap of the rows (built on the first call per `axes`, and kept): with the default axes voxel_to_bev gives
        [B, C * Z, Y, X]"""
        key = tuple(axes) if isinstance(axes, (tuple, list)) else axes
        dmap = self._dense.get(key)
        if dmap is None:
            with torch.cuda.device(self.device):
                dmap = self._dense[key] = VoxelDenseMap(self.coords, self.shape, self.batch_index, self.batch_size, axes=axes)
        return dmap


def _forward(depth, feat, fmap):
    """depth [S, D, H, W], feat [S, H, W, C] on fmap.device -> [V, C]; one launch"""
    (d, h, w), c, v = fmap.frustum, feat.shape[-1], fmap.num_voxels
    with torch.cuda.device(fmap.device):
        if v == 0 or c == 0:
            return feat.new_zeros((v, c))
        out = torch.empty((v, c), dtype=feat.dtype, device=fmap.device)
        rc = _lib.load().d3d_lift_pool_forward(_lib.ptr(depth), _lib.ptr(feat), fmap.num_cameras, d, h, w, c, FEATURE_CODES[feat.dtype],
                                               _lib.ptr(fmap.index.order), _lib.ptr(fmap.index.offsets), v, _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "lift_splat")
    return out


def _backward_feat(grad, depth, fmap):
    """grad [V, C], depth [S, D, H, W] on fmap.device -> [S, H, W, C]; one gather launch, every row written once"""
    (d, h, w), c, s = fmap.frustum, grad.shape[1], fmap.num_cameras
    with torch.cuda.device(fmap.device):
        if s * h * w * c == 0 or fmap.num_voxels == 0:
            return grad.new_zeros((s, h, w, c))
        out = torch.empty((s, h, w, c), dtype=grad.dtype, device=fmap.device)
        rc = _lib.load().d3d_lift_pool_backward_feat(_lib.ptr(grad), fmap.num_voxels, _lib.ptr(depth), _lib.ptr(fmap.mapping), s, d, h, w, c,
                                                     FEATURE_CODES[grad.dtype], _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "lift_splat backward (feat)")
    return out


def _backward_depth(grad, feat, fmap):
    """grad [V, C], feat [S, H, W, C] on fmap.device -> [S, D, H, W]; one launch"""
    (d, h, w), c, s = fmap.frustum, grad.shape[1], fmap.num_cameras
    with torch.cuda.device(fmap.device):
        if fmap.num_points == 0 or c == 0 or fmap.num_voxels == 0:
            return grad.new_zeros((s, d, h, w))
        out = torch.empty((s, d, h, w), dtype=grad.dtype, device=fmap.device)
        rc = _lib.load().d3d_lift_pool_backward_depth(_lib.ptr(grad), fmap.num_voxels, _lib.ptr(feat), _lib.ptr(fmap.mapping), s, d, h, w, c,
                                                      FEATURE_CODES[grad.dtype], _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "lift_splat backward (depth)")
    return out


class LiftSplat(torch.autograd.Function):
    """lift_splat: (depth [S, D, H, W], feat [S, H, W, C], FrustumMap) -> [V, C].  One launch forward; backward one launch per
    gradient that is needed (feat: a gather over the depth bins of every pixel; depth: a dot product per point).  Differentiable once."""

    @staticmethod
    def forward(ctx, depth, feat, fmap):
        ctx.fmap, ctx.odev, ctx.shapes = fmap, feat.device, (depth.shape, feat.shape)
        d, f = to_owner(depth, fmap), to_owner(feat, fmap)
        need_depth, need_feat = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.save_for_backward(f if need_depth else None, d if need_feat else None)
        return _lib.to_caller(_forward(d, f, fmap), ctx.odev, fmap.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        fmap = ctx.fmap
        f, d = ctx.saved_tensors
        g = to_owner(grad, fmap)
        gd = gf = None
        if ctx.needs_input_grad[0]:
            gd = _lib.to_caller(_backward_depth(g, f, fmap), ctx.odev, fmap.device).reshape(ctx.shapes[0])
        if ctx.needs_input_grad[1]:
            gf = _lib.to_caller(_backward_feat(g, d, fmap), ctx.odev, fmap.device).reshape(ctx.shapes[1])
        return gd, gf, None


def _front(depth, feat, fmap):
    if not isinstance(fmap, FrustumMap):
        raise TypeError("fmap must be a FrustumMap")
    depth, dn = as_tensor(depth, "depth")
    feat, fn = as_tensor(feat, "feat")
    dtype_code(feat, FEATURE_CODES, "feat")
    if depth.dtype != feat.dtype:
        raise ValueError("depth and feat must have one dtype, not %s and %s" % (depth.dtype, feat.dtype))
    (d, h, w), s, b, n = fmap.frustum, fmap.num_cameras, fmap.batch_size, fmap.cams_per_sample
    if tuple(depth.shape) not in ((s, d, h, w), (b, n, d, h, w)):
        raise ValueError("depth has the shape %r where the FrustumMap expects %r (or the cameras as [B, N])" % (tuple(depth.shape), (s, d, h, w)))
    if tuple(feat.shape[:-1]) not in ((s, h, w), (b, n, h, w)):
        raise ValueError("feat has the shape %r where the FrustumMap expects %r (channels last; or the cameras as [B, N])"
                         % (tuple(feat.shape), (s, h, w, "C")))
    if depth.device != feat.device:
        raise ValueError("depth lives on %s, feat on %s" % (depth.device, feat.device))
    check_owner_device(fmap, feat)
    return depth, feat, dn and fn


def lift_splat(depth, feat, fmap):
    """Sum depth-weighted camera features into the cells of the ego grid.

    :param depth: [S, D, H, W] (or [B, N, D, H, W]) float32, float64, float16 or bfloat16; torch tensor (GPU or host) or numpy array;
        differentiable (once)
    :param feat: [S, H, W, C] (or [B, N, H, W, C]), channels LAST, the dtype and side of depth; differentiable (once)
    :param fmap: the FrustumMap of the frame
    :return: [V, C] on the side the inputs came from, row r = 0 + depth[p] * feat[pixel(p)] over the points p of cell r in ascending p,
        product and sum rounded separately (half types: in fp32, one rounding at the end): the left fold index_add_ would compute on one
        thread.  grad_feat follows the same rule over the depth bins of a pixel in ascending d, bit for bit; grad_depth is a dot
        product over the channels in fp32 (fp64 for float64) whose order is the kernel's own.  Each gradient is computed only when its
        input needs it.  The geometry gets none
    """
    depth, feat, was_numpy = _front(depth, feat, fmap)
    return back_to_caller(LiftSplat.apply(depth, feat, fmap), was_numpy)


def lift_splat_bev(depth, feat, fmap):
    """voxel_to_bev(lift_splat(depth, feat, fmap), fmap.dense_map()): the BEV map [B, C * Z, Y, X], zero where no point lands"""
    return voxel_to_bev(lift_splat(depth, feat, fmap), fmap.dense_map())


def frustum_matrices(rots, trans, intrins, post_rots, post_trans, extra_rots=None, extra_trans=None):
    """The two affine maps of a FrustumMap from the calibrations, LSS's get_geometry with BEVFusion's extra LiDAR augmentation folded in:
    a frustum point (u, v, d) goes through q = post_rots^-1 ((u, v, d) - post_trans), e = (q0 * q2, q1 * q2, q2),
    x = E (rots intrins^-1 e + trans) + extra_trans.

    :param rots, intrins, post_rots: [..., 3, 3]; trans, post_trans: [..., 3] -- camera to ego, the intrinsics, the image augmentation;
        any leading dimensions ([S] or [B, N]), the same for all five
    :param extra_rots, extra_trans: [..., 3, 3] / [..., 3] or None (identity / zero), with the leading dimensions of the others or one
        fewer ([B] beside [B, N]: one per sample)
    :return: (pre, post), each [S, 3, 4] float32: pre = [post_rots^-1 | -post_rots^-1 post_trans], post = [E rots intrins^-1 | E trans +
        extra_trans], computed in fp64 on the host and rounded ONCE to fp32; numpy arrays when everything came as numpy, else host tensors
    """
    given = [rots, trans, intrins, post_rots, post_trans] + [x for x in (extra_rots, extra_trans) if x is not None]
    all_numpy = all(isinstance(x, np.ndarray) for x in given)

    def f64(x, what, tail):
        x, _ = as_tensor(x, what)
        a = x.detach().cpu().to(torch.float64).numpy()
        if a.ndim < len(tail) or a.shape[a.ndim - len(tail):] != tail:
            raise ValueError("%s must end in the shape %r, not %r" % (what, tail, a.shape))
        return a

    rots, intrins, post_rots = (f64(x, n, (3, 3)) for x, n in ((rots, "rots"), (intrins, "intrins"), (post_rots, "post_rots")))
    trans, post_trans = f64(trans, "trans", (3,)), f64(post_trans, "post_trans", (3,))
    lead = rots.shape[:-2]
    if any(x.shape[:-2] != lead for x in (intrins, post_rots)) or any(x.shape[:-1] != lead for x in (trans, post_trans)):
        raise ValueError("rots, trans, intrins, post_rots and post_trans must share their leading dimensions")
    e_rot = np.broadcast_to(np.eye(3), lead + (3, 3)) if extra_rots is None else f64(extra_rots, "extra_rots", (3, 3))
    e_tr = np.zeros(lead + (3,)) if extra_trans is None else f64(extra_trans, "extra_trans", (3,))
    if e_rot.shape[:-2] == lead[:-1] and len(lead) >= 1 and e_rot.shape[:-2] != lead:
        e_rot = np.broadcast_to(e_rot[..., None, :, :], lead + (3, 3))
    if e_tr.shape[:-1] == lead[:-1] and len(lead) >= 1 and e_tr.shape[:-1] != lead:
        e_tr = np.broadcast_to(e_tr[..., None, :], lead + (3,))
    if e_rot.shape[:-2] != lead or e_tr.shape[:-1] != lead:
        raise ValueError("extra_rots / extra_trans must have the leading dimensions of rots, or one fewer")
    inv_post = np.linalg.inv(post_rots)
    pre = np.concatenate([inv_post, -(inv_post @ post_trans[..., None])], -1)
    post = np.concatenate([e_rot @ (rots @ np.linalg.inv(intrins)), e_rot @ trans[..., None] + e_tr[..., None]], -1)
    pre, post = (np.ascontiguousarray(m.reshape(-1, 3, 4).astype(np.float32)) for m in (pre, post))
    return (pre, post) if all_numpy else (torch.from_numpy(pre), torch.from_numpy(post))


__all__ = ["FrustumMap", "lift_splat", "lift_splat_bev", "frustum_matrices", "LiftSplat", "grid_of"]
