"""The numpy model of d3d_amd.voxel.pool (VoxelIndex / voxel_pool / voxel_unpool): the index definition, the left folds, the
comparators and the backward rules, written from the operator's contract and from nothing else.

The folds run rank by rank: step r handles the r-th point (in point order) of every voxel at once -- at most one point per voxel
and step, so `acc[voxels] = acc[voxels] + f[points]` is the strict left fold of every voxel, in the array's dtype."""
import numpy as np

REDUCTIONS = ("sum", "mean", "max", "min")


def index(mapping, v):
    """-> (order [K'] int32, offsets [V+1] int64): the mapped points by ascending voxel id, ascending point index inside a voxel"""
    m = np.asarray(mapping, dtype=np.int64)
    assert np.all((m >= -1) & (m < v))
    kept = np.nonzero(m >= 0)[0]
    order = kept[np.argsort(m[kept], kind="stable")].astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(m[kept], minlength=v))]).astype(np.int64)
    return order, offsets


def _steps(m, v):
    """yields (points, voxels) of fold step 0, 1, ...: the points of rank r inside their voxel"""
    order, offsets = index(m, v)
    vox = m[order]
    rank = np.arange(len(order)) - offsets[vox]
    by_rank = np.argsort(rank, kind="stable")
    cuts = np.concatenate([[0], np.cumsum(np.bincount(rank))]) if len(order) else [0]
    for r in range(len(cuts) - 1):
        sel = by_rank[cuts[r]:cuts[r + 1]]
        yield order[sel].astype(np.int64), vox[sel]


def pool(f, mapping, v, reduction):
    """-> (out [V, C] in f's dtype, arg [V, C] int32: the winner's point index for max / min, -1 for an empty voxel; None for
    sum / mean)"""
    f = np.asarray(f)
    m = np.asarray(mapping, dtype=np.int64)
    c = f.shape[1]
    acc = np.zeros((v, c), f.dtype)
    if reduction in ("sum", "mean"):
        with np.errstate(invalid="ignore"):                      # (+inf + -inf)
            for pts, vox in _steps(m, v):
                acc[vox] = acc[vox] + f[pts]
        if reduction == "mean":
            cnt = np.diff(index(m, v)[1])
            acc = np.where((cnt > 0)[:, None], acc / np.maximum(cnt, 1).astype(f.dtype)[:, None], acc).astype(f.dtype)
        return acc, None
    arg = np.full((v, c), -1, np.int32)
    with np.errstate(invalid="ignore"):
        for pts, vox in _steps(m, v):
            x, best = f[pts], acc[vox]
            beats = (x > best) if reduction == "max" else (x < best)
            take = (arg[vox] < 0) | (~np.isnan(best) & (beats | np.isnan(x)))
            acc[vox] = np.where(take, x, best)
            arg[vox] = np.where(take, pts[:, None].astype(np.int32), arg[vox])
    return acc, arg


def backward(grad, mapping, v, reduction, arg=None):
    """grad [V, C] -> [K, C]: the gradient of pool(...) with respect to the features"""
    grad = np.asarray(grad)
    m = np.asarray(mapping, dtype=np.int64)
    out = np.zeros((len(m), grad.shape[1]), grad.dtype)
    pts = np.nonzero(m >= 0)[0]
    g = grad[m[pts]]
    if reduction == "mean":
        cnt = np.diff(index(m, v)[1])
        g = g / cnt[m[pts]].astype(grad.dtype)[:, None]
    elif reduction in ("max", "min"):
        g = np.where(arg[m[pts]] == pts[:, None], g, np.zeros_like(g))
    out[pts] = g
    return out


def unpool(voxel_features, mapping):
    vf = np.asarray(voxel_features)
    return backward(vf, mapping, vf.shape[0], "sum")


def same_bits(a, b):
    """bit for bit, -0.0 apart from +0.0; any NaN equals any NaN (a sum's NaN carries no promised payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.all((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))))
