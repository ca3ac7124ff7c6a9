"""d3d_amd.voxel.sparse_pool -- pooling through the tables of the sparse convolutions (spconv's SparseMaxPool3d / SparseAvgPool3d):
the max-pool downsampling of sparse U-Nets and PV-RCNN-style heads, and stride-1 "same" pooling over a voxel's neighbourhood.  An
extension (the reference stops at the voxelizer).

    cmap = SparseConvMap(sp.coords, kernel_size=3, stride=2, padding=1)      # the map a strided convolution would use
    y    = sparse_max_pool3d(vf, cmap)                           # [Vout, C]: row r belongs to cmap.out_coords[r]
    z    = sparse_pool3d(vf, VoxelNeighbors(sp.coords), "mean")  # [V, C]: over the active neighbours of every voxel

Only the ACTIVE inputs of a window take part: an absent neighbour is not a zero, so a max over negative features stays negative
and a mean divides by the number of active inputs.  The two tables of a map are each other's transposed map, so the gradient is
again a gather: one launch forward, one backward, no [rows, K, C] buffer, no float atomics, in fp32, fp64, fp16 and bf16 (kernels
and the exact rules: csrc/vtpool.hip, include/d3d_hip.h).
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._rows import FEATURE_CODES, as_tensor, back_to_caller, check_rows, on_owner
from .conv import VoxelNeighbors
from .pool import EXTREME, REDUCTIONS
from .sparse_conv import SparseConvMap


def _pool_forward(feat, view, red, need_arg, need_count):
    """feat [view.src_rows, C] on view.device -> (out [rows, C], arg [rows, C] int16 or None, count [rows] int32 or None); one launch"""
    rows, c = view.num_voxels, feat.shape[1]
    with torch.cuda.device(view.device):
        out = torch.empty((rows, c), dtype=feat.dtype, device=view.device)
        arg = torch.empty((rows, c), dtype=torch.int16, device=view.device) if need_arg else None
        count = torch.empty((rows,), dtype=torch.int32, device=view.device) if need_count else None
        if rows and c:
            rc = _lib.load().d3d_table_pool_forward(_lib.ptr(feat), view.src_rows, c, FEATURE_CODES[feat.dtype], _lib.ptr(view.table), rows,
                                                    view.kernel_volume, red, _lib.ptr(out), _lib.ptr(arg), _lib.ptr(count), _lib.stream_ptr())
            _lib.check(rc, "table_pool")
    return out, arg, count


def _pool_backward(grad, view, mirrored, red, arg, count):
    """grad [view.src_rows, C] on view.device -> [rows, C] through the BACKWARD view; one launch, every row written once"""
    rows, c = view.num_voxels, grad.shape[1]
    with torch.cuda.device(view.device):
        if rows == 0 or c == 0 or view.src_rows == 0:
            return grad.new_zeros((rows, c))
        out = torch.empty((rows, c), dtype=grad.dtype, device=view.device)
        rc = _lib.load().d3d_table_pool_backward(_lib.ptr(grad), view.src_rows, c, FEATURE_CODES[grad.dtype], _lib.ptr(view.table), rows,
                                                 view.kernel_volume, int(mirrored), red, _lib.ptr(arg), _lib.ptr(count), _lib.ptr(out),
                                                 _lib.stream_ptr())
    _lib.check(rc, "table_pool backward")
    return out


class TablePool(torch.autograd.Function):
    """sparse_pool3d: (features [fwd.src_rows, C], the forward and the backward view of one map, whether the backward view is read
    mirrored, the reduction code) -> [fwd.num_voxels, C], one launch.  Saves the winners' columns (int16) for max / min and the counts
    for mean when the features need a gradient; backward is one launch through the other view.  Differentiable once."""

    @staticmethod
    def forward(ctx, features, fwd, bwd, bwd_mirrored, red):
        need = ctx.needs_input_grad[0]
        out, arg, count = on_owner(_pool_forward, features, fwd, features.device, red, need and red in EXTREME,
                                   need and red == _lib.REDUCE_MEAN)
        if need:
            ctx.bwd, ctx.bwd_mirrored, ctx.red, ctx.odev = bwd, bwd_mirrored, red, features.device
            ctx.save_for_backward(*[t for t in (arg, count) if t is not None])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        saved = ctx.saved_tensors[0] if ctx.saved_tensors else None
        arg, count = (saved, None) if ctx.red in EXTREME else (None, saved)
        return on_owner(_pool_backward, grad, ctx.bwd, ctx.odev, ctx.bwd_mirrored, ctx.red, arg, count), None, None, None, None


def sparse_pool3d(features, where, reduction="max"):
    """Pool the rows of the active voxels through the table of a convolution.

    :param features: [V, C] float32, float64, float16 or bfloat16, torch tensor (GPU or host) or numpy array; differentiable (once)
    :param where: a SparseConvMap -- [V, C] -> [Vout, C], row r belongs to where.out_coords[r] and reduces the inputs inside the
        window of that output (kernel size, stride, padding and dilation are the map's) -- or a VoxelNeighbors -- [V, C] -> [V, C],
        stride-1 "same" pooling over the active neighbours of every voxel, itself included
    :param reduction: 'max' | 'min' | 'sum' | 'mean' (any case)
    :return: the pooled rows on the side features came from.  Only the active inputs count (an absent one is not a zero): sum is
        the left fold 0 + x_0 + x_1 + ... in ascending column of the table, mean that sum / the number of active inputs, max / min the
        first strict winner in that order, NaN propagates (the first one wins).  Half types sum and divide in fp32 and round once.
        A row's bits depend on its window alone, and every run gives the same bits.  The gradient goes to the winner (max / min,
        ties: the lowest column), to every input (sum), divided by the count (mean), summed per input in ascending column of the
        other table
    """
    if isinstance(where, SparseConvMap):
        fwd, bwd, mirrored = where._down, where._up, False
    elif isinstance(where, VoxelNeighbors):
        fwd, bwd, mirrored = where._view, where._view, True
    else:
        raise TypeError("where must be a SparseConvMap or a VoxelNeighbors")
    if not isinstance(reduction, str) or reduction.lower() not in REDUCTIONS:
        raise ValueError("Unsupported reduction %r in sparse_pool3d: sum, mean, max or min" % (reduction,))
    features, was_numpy = as_tensor(features, "features")
    check_rows(features, "features", "voxel", "voxel features", FEATURE_CODES, where, fwd.src_rows)
    out = TablePool.apply(features, fwd, bwd, mirrored, REDUCTIONS[reduction.lower()])
    return back_to_caller(out, was_numpy)


def sparse_max_pool3d(features, where):
    """sparse_pool3d(features, where, "max"): spconv's SparseMaxPool3d"""
    return sparse_pool3d(features, where, "max")


def sparse_avg_pool3d(features, where):
    """sparse_pool3d(features, where, "mean"): the mean over the ACTIVE inputs of every window (spconv's SparseAvgPool3d)"""
    return sparse_pool3d(features, where, "mean")


__all__ = ["sparse_pool3d", "sparse_max_pool3d", "sparse_avg_pool3d", "TablePool"]
