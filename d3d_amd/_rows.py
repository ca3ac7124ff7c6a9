"""d3d_amd._rows -- what every operator on rows needs, once: the voxel operators of d3d_amd.voxel (pool, conv, sparse_conv, sparse_pool,
interp, dense) and the point operators of d3d_amd.point (sample, knn) take feature or coordinate rows [N, C] as a torch tensor (GPU
or host) or a numpy array, check them against an owner built once per frame (a VoxelIndex, VoxelNeighbors, SparseConvMap, VoxelInterp,
VoxelDenseMap or PointInterp: anything with a `device`), run on the owner's GPU and answer on the caller's side.  The limits and
dtype tables, that ingress and egress, and the autograd function of an operator whose gradient is its transpose live here; the
operator modules take them from here and not from each other."""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib

ROW_MAX = 2 ** 31 - 1               # rows, voxels and table entries are numbered in int32
FLOAT_CODES = {torch.float32: _lib.F32, torch.float64: _lib.F64}                         # coordinates, positions, weights
FEATURE_CODES = {**FLOAT_CODES, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}     # feature rows


def as_tensor(x, what):
    """-> (x as a tensor, whether it came as a numpy array)"""
    if isinstance(x, np.ndarray):
        return torch.from_numpy(x), True
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor or numpy array" % what)
    return x, False


def back_to_caller(out, was_numpy):
    return out.detach().numpy() if was_numpy else out


def device_of(*xs):
    """the device of the first argument that is a tensor on a GPU (anything else is skipped), else the current GPU"""
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return _lib.require_gpu()


def check_owner_device(owner, t):
    """a tensor already on a GPU must be on the one its owner was built on"""
    if t.is_cuda and t.device != owner.device:
        raise ValueError("features live on %s, the %s on %s" % (t.device, type(owner).__name__, owner.device))


def dtype_code(t, codes, subject):
    """the library's code of t's dtype; ValueError for one outside `codes` (FLOAT_CODES or FEATURE_CODES)"""
    code = codes.get(t.dtype)
    if code is None:
        names = [str(d).replace("torch.", "") for d in codes]
        raise ValueError("%s must be %s or %s, not %s" % (subject, ", ".join(names[:-1]), names[-1], t.dtype))
    return code


def check_rows(t, name, row, subject, codes, owner=None, rows=None):
    """The checks of a front on its rows, in their order: 2-D ("one row per `row`"), a dtype of `codes` (`subject` is what the
    message calls the rows), and with an owner: `rows` of them, and on the owner's GPU when on one at all."""
    if t.dim() != 2:
        raise ValueError("%s must be a 2-D tensor of one row per %s" % (name, row))
    dtype_code(t, codes, subject)
    if owner is not None:
        if t.shape[0] != rows:
            raise ValueError("%s has %d rows where the %s expects %d" % (name, t.shape[0], type(owner).__name__, rows))
        check_owner_device(owner, t)


def check_xyz_rows(t, what):
    """coordinate rows of the point operators: [N, D] with D >= 3, float32 or float64"""
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError("%s must be [N, D] with D >= 3 (columns 0..2 are the coordinates), not %s" % (what, tuple(t.shape)))
    if t.dtype not in FLOAT_CODES:
        raise ValueError("%s must be float32 or float64, not %s" % (what, t.dtype))


def host_offsets(offsets, total, what):
    """offsets -> a list of ints [B + 1], checked: 1-D, from 0 to `total`, nondecreasing.  None: one segment.  Offsets belong on the
    host; a GPU tensor is read back (one blocking copy) for the checks."""
    if offsets is None:
        offsets = [0, int(total)]
    if isinstance(offsets, torch.Tensor):
        if offsets.dim() != 1 or offsets.dtype not in (torch.int64, torch.int32):
            raise ValueError("%s must be a 1-D int64 or int32 tensor" % what)
        offs = offsets.cpu().tolist()                    # (a GPU tensor: the read-back)
    else:
        arr = np.asarray(offsets)
        if arr.ndim != 1 or (arr.size and not np.issubdtype(arr.dtype, np.integer)):
            raise ValueError("%s must be a 1-D sequence of integers" % what)
        offs = [int(v) for v in arr.tolist()]
    if len(offs) < 1 or offs[0] != 0 or offs[-1] != int(total) or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError("%s must run nondecreasing from 0 to %d (the number of rows)" % (what, int(total)))
    if any(b - a > ROW_MAX for a, b in zip(offs, offs[1:])):
        raise ValueError("a segment of %s holds more than 2^31 - 1 rows" % what)
    return offs


def group_ids(groups):
    """groups as an int64 torch tensor whose equal values are the caller's equal values (uint64 is reinterpreted: a bijection)"""
    if isinstance(groups, np.ndarray):
        if not np.issubdtype(groups.dtype, np.integer):
            raise TypeError("groups must be an integer array, got %s" % groups.dtype)
        groups = np.ascontiguousarray(groups)
        return torch.from_numpy(groups.view(np.int64) if groups.dtype == np.uint64 else groups.astype(np.int64, copy=False))
    if not torch.is_tensor(groups):
        raise TypeError("groups must be a torch tensor or a numpy array of integers")
    if groups.dtype == torch.bool or groups.is_floating_point() or groups.is_complex():
        raise TypeError("groups must be an integer tensor, got %s" % groups.dtype)
    if groups.dtype == getattr(torch, "uint64", None):
        return groups.contiguous().view(torch.int64)
    return groups.to(torch.int64)


def rows_on(t, dev):
    """-> (tensor on dev with unit column stride, its row stride in elements)"""
    t = t.detach().to(dev)
    if t.shape[0] > 1 and t.stride(1) == 1 and t.shape[1] <= t.stride(0) <= ROW_MAX:      # a column slice of wider rows: as it lies
        return t, int(t.stride(0))
    return t.contiguous(), int(t.shape[1])


def to_owner(x, owner):
    """x as a kernel of the owner reads it: detached, on the owner's GPU, contiguous"""
    return x.detach().to(owner.device).contiguous()


def on_owner(op, x, owner, odev, *args):
    """op(x on the owner's GPU, owner, *args), its result back on the caller's device `odev`: the forward of an operator and, with
    the incoming gradient for x, its backward.  Where op returns a tuple, its first element is the result and goes back; the others
    (what a backward needs: winners, counts) stay where they are."""
    out = op(to_owner(x, owner), owner, *args)
    if isinstance(out, tuple):
        return (_lib.to_caller(out[0], odev, owner.device),) + out[1:]
    return _lib.to_caller(out, odev, owner.device)


class TransposePair(torch.autograd.Function):
    """(x, owner, op, transposed op) -> op(x, owner); its gradient is the transposed op of the incoming gradient, and nothing is
    saved: an interpolation and its splat, a scatter into a dense grid and the gather out of it.  Differentiable once, in x only."""

    @staticmethod
    def forward(ctx, x, owner, op, op_t):
        ctx.owner, ctx.op_t, ctx.odev = owner, op_t, x.device
        return on_owner(op, x, owner, ctx.odev)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return on_owner(ctx.op_t, grad, ctx.owner, ctx.odev), None, None, None
