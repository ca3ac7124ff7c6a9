"""d3d_amd.voxel.pool -- per-voxel pooling of learned point features (point -> voxel) and its inverse gather (voxel -> point),
both differentiable: what a dynamic VFE / PillarFeatureNet / PointNet-style voxel encoder does first with the voxelizer's output.
An extension (the reference reduces the raw input columns inside its voxelizer only, without a gradient).

    sp  = VoxelGenerator(bounds, shape, max_points=32, max_points_filter="trim")(pts)    # sparse contract
    idx = VoxelIndex(sp.points_mapping, sp.coords.shape[0])      # once per frame; every layer and every backward reuses it
    v   = voxel_pool(mlp(sp.points), idx, reduction="max")       # [V, C]
    f2  = voxel_unpool(v, idx)                                   # [K, C]: the voxel's row on each of its points

No float atomics: the index groups the points by voxel (stable, in point order) and the kernels fold a voxel's rows strictly in
that order, so the results are the same bits on every run (kernels and the exact rules: csrc/vpool.hip, include/d3d_hip.h).
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._rows import FLOAT_CODES, ROW_MAX, as_tensor, back_to_caller, check_owner_device, check_rows, device_of, dtype_code, on_owner

REDUCTIONS = {"sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_MEAN, "max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN}     # (sparse_pool's too)
EXTREME = (_lib.REDUCE_MAX, _lib.REDUCE_MIN)


def _dtype_code(t):
    return dtype_code(t, FLOAT_CODES, "voxel features")


class VoxelIndex:
    """The inverted mapping of one frame: which points each voxel holds.

    :param mapping: [K] int64 (int32 is widened) voxel id of every point in [0, num_voxels), or -1 for "belongs to no voxel"
        (`points_mapping` of the sparse VoxelGenerator); torch tensor or numpy array, on the GPU or the host
    :param num_voxels: V
    :param keep_mapping: False: `mapping` is None once the index is built -- for an owner that has the mapping in another form and
        only folds through `order` / `offsets` (VoxelInterp: the widened copy of its int32 table would stay for the whole frame);
        voxel_unpool and the backward of voxel_pool need it

    Holds `mapping` [K] int64, `order` [K'] int32 (the mapped points by ascending voxel id, ascending point index inside a voxel),
    `offsets` [V+1] int64 (CSR) and `num_mapped` = K', all on the GPU.  Building it reads two numbers back (K' and the count of
    ids outside [-1, V): ValueError if that is not 0); no pooling call reads anything back."""

    def __init__(self, mapping, num_voxels, keep_mapping=True):
        mapping, _ = as_tensor(mapping, "mapping")
        if mapping.dim() != 1:
            raise ValueError("mapping must be a [K] tensor of voxel ids")
        if mapping.dtype not in (torch.int64, torch.int32):
            raise ValueError("mapping must be int64 or int32, not %s" % mapping.dtype)
        v, k = int(num_voxels), mapping.shape[0]
        if v < 0:
            raise ValueError("num_voxels must not be negative")
        if k > ROW_MAX or v > ROW_MAX:
            raise ValueError("voxel_pool takes at most 2^31 - 1 points and voxels")
        dev = device_of(mapping)
        self.device, self.num_voxels, self.num_points = dev, v, k
        self.mapping = mapping.to(device=dev, dtype=torch.int64).contiguous()
        with torch.cuda.device(dev):
            self.offsets = torch.zeros((v + 1,), dtype=torch.int64, device=dev)
            if k == 0 or v == 0:                         # nothing to launch; ids other than -1 are still refused
                bad = int((self.mapping != -1).sum()) if k else 0
                mapped, order = 0, torch.empty((0,), dtype=torch.int32, device=dev)
            else:
                lib = _lib.load()
                order = torch.empty((k,), dtype=torch.int32, device=dev)
                counts = torch.empty((2,), dtype=torch.int64, device=dev)
                nbytes = lib.d3d_voxel_index_workspace_bytes(k, v)
                ws = _lib.workspace(nbytes, dev)
                rc = lib.d3d_voxel_index(_lib.ptr(self.mapping), k, v, _lib.ptr(order), _lib.ptr(self.offsets), _lib.ptr(counts),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
                _lib.check(rc, "voxel_index")
                mapped, bad = counts.tolist()            # the one read-back of a frame's index
        if bad:
            raise ValueError("mapping holds %d voxel ids outside [-1, %d)" % (bad, v))
        self.num_mapped = mapped
        self.order = order[:mapped]
        if not keep_mapping:
            self.mapping = None


def _index_of(index_or_mapping, num_voxels):
    if isinstance(index_or_mapping, VoxelIndex):
        if num_voxels is not None and int(num_voxels) != index_or_mapping.num_voxels:
            raise ValueError("num_voxels = %d, the VoxelIndex was built for %d" % (int(num_voxels), index_or_mapping.num_voxels))
        return None, index_or_mapping
    if num_voxels is None:
        raise ValueError("num_voxels is required with a bare mapping")
    return index_or_mapping, None


def _beside(mapping, features):
    """a bare mapping goes to the GPU the features live on (host features: the current device, as everywhere)"""
    mapping, _ = as_tensor(mapping, "mapping")
    return mapping.to(features.device) if features.is_cuda else mapping


def _forward(feat, idx, red, need_arg):
    """features [K, C] on idx.device -> (out [V, C], arg [V, C] int32 or None); one launch"""
    k, c = feat.shape
    v = idx.num_voxels
    with torch.cuda.device(idx.device):
        if v == 0 or c == 0:
            return feat.new_zeros((v, c)), None
        if k == 0 or idx.num_mapped == 0:
            return feat.new_zeros((v, c)), (torch.full((v, c), -1, dtype=torch.int32, device=idx.device) if need_arg else None)
        out = torch.empty((v, c), dtype=feat.dtype, device=idx.device)
        arg = torch.empty((v, c), dtype=torch.int32, device=idx.device) if need_arg else None
        rc = _lib.load().d3d_voxel_pool_forward(_lib.ptr(feat), k, c, _dtype_code(feat), _lib.ptr(idx.order), _lib.ptr(idx.offsets), v,
                                                red, _lib.ptr(out), _lib.ptr(arg), _lib.stream_ptr())
    _lib.check(rc, "voxel_pool")
    return out, arg


def _backward(grad, idx, red, arg):
    """grad [V, C] on idx.device -> [K, C]; one launch, every row written once"""
    v, c = grad.shape
    k = idx.num_points
    with torch.cuda.device(idx.device):
        if k == 0 or c == 0 or v == 0:
            return grad.new_zeros((k, c))
        out = torch.empty((k, c), dtype=grad.dtype, device=idx.device)
        rc = _lib.load().d3d_voxel_pool_backward(_lib.ptr(grad), v, c, _dtype_code(grad), _lib.ptr(idx.mapping), k, _lib.ptr(idx.offsets),
                                                 red, _lib.ptr(arg), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "voxel_pool backward")
    return out


class VoxelPool(torch.autograd.Function):
    """voxel_pool: (features [K, C], VoxelIndex, reduction code) -> [V, C].  One launch; max / min also write the winners' point
    indices when the features need a gradient.  backward is one gather launch.  Differentiable once."""

    @staticmethod
    def forward(ctx, features, idx, red):
        need = ctx.needs_input_grad[0]
        out, arg = on_owner(_forward, features, idx, features.device, red, need and red in EXTREME)
        if need:
            ctx.idx, ctx.red, ctx.odev = idx, red, features.device
            ctx.save_for_backward(*([arg] if arg is not None else []))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        arg = ctx.saved_tensors[0] if ctx.saved_tensors else None
        return on_owner(_backward, grad, ctx.idx, ctx.odev, ctx.red, arg), None, None


class VoxelUnpool(torch.autograd.Function):
    """voxel_unpool: (voxel features [V, C], VoxelIndex) -> [K, C]; forward is the `sum` backward kernel, backward the `sum`
    forward kernel.  Differentiable once."""

    @staticmethod
    def forward(ctx, voxel_features, idx):
        ctx.idx, ctx.odev = idx, voxel_features.device
        return on_owner(_backward, voxel_features, idx, ctx.odev, _lib.REDUCE_SUM, None)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return on_owner(_forward, grad, ctx.idx, ctx.odev, _lib.REDUCE_SUM, False)[0], None


def voxel_pool(features, index_or_mapping, num_voxels=None, reduction="max"):
    """Reduce per-point feature rows into their voxels.

    :param features: [K, C] float32 or float64, torch tensor (GPU or host) or numpy array; differentiable (once)
    :param index_or_mapping: a VoxelIndex (build it once per frame), or the [K] mapping itself (an index is built for this call)
    :param num_voxels: V; required with a bare mapping
    :param reduction: 'sum' | 'mean' | 'max' | 'min' (any case)
    :return: [V, C] on the caller's device.  sum: the left fold 0 + x_0 + x_1 + ... over the voxel's points in ascending point
        index, in the dtype (np.add.at's bits); mean: that sum / count; max / min: the first strict winner in point order, NaN
        propagates (the first one wins); a voxel without points gives 0
    """
    if not isinstance(reduction, str) or reduction.lower() not in REDUCTIONS:
        raise ValueError("Unsupported reduction %r in voxel_pool: sum, mean, max or min" % (reduction,))
    red = REDUCTIONS[reduction.lower()]
    features, was_numpy = as_tensor(features, "features")
    check_rows(features, "features", "point", "voxel features", FLOAT_CODES)
    mapping, idx = _index_of(index_or_mapping, num_voxels)
    k = idx.num_points if idx is not None else len(mapping)
    if features.shape[0] != k:
        raise ValueError("features has %d rows, the mapping %d points" % (features.shape[0], k))
    if idx is None:
        idx = VoxelIndex(_beside(mapping, features), num_voxels)
    check_owner_device(idx, features)
    out = VoxelPool.apply(features, idx, red)
    return back_to_caller(out, was_numpy)


def voxel_unpool(voxel_features, index_or_mapping, num_voxels=None):
    """Each point gets the row of its voxel: row i of the result is voxel_features[mapping[i]], zero where mapping[i] == -1.

    :param voxel_features: [V, C] float32 or float64; differentiable (once)
    :param index_or_mapping: a VoxelIndex, or the [K] mapping itself
    :return: [K, C] on the caller's device
    """
    voxel_features, was_numpy = as_tensor(voxel_features, "voxel_features")
    check_rows(voxel_features, "voxel_features", "voxel", "voxel features", FLOAT_CODES)
    mapping, idx = _index_of(index_or_mapping, voxel_features.shape[0] if num_voxels is None else num_voxels)
    if idx is None:
        idx = VoxelIndex(_beside(mapping, voxel_features), voxel_features.shape[0])
    if voxel_features.shape[0] != idx.num_voxels:
        raise ValueError("voxel_features has %d rows, the index %d voxels" % (voxel_features.shape[0], idx.num_voxels))
    check_owner_device(idx, voxel_features)
    out = VoxelUnpool.apply(voxel_features, idx)
    return back_to_caller(out, was_numpy)


__all__ = ["VoxelIndex", "voxel_pool", "voxel_unpool", "VoxelPool", "VoxelUnpool"]
