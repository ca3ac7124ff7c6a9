"""d3d_amd.voxel._coords -- the checks of voxel coordinates and of per-axis parameters that every owner built from coords shares:
VoxelNeighbors (conv), SparseConvMap (sparse_conv), VoxelInterp (interp) and VoxelDenseMap (dense).  Nothing here needs a GPU."""
import numpy as np
import torch

from .._rows import as_tensor

_SPAN_LIMIT = 2 ** 62


def _triple(x, what):
    t = tuple(x) if isinstance(x, (tuple, list)) else (x, x, x)
    if len(t) != 3 or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in t):
        raise ValueError("%s must be an int or three ints, not %r" % (what, x))
    return tuple(int(a) for a in t)


def _host_spans_fit(coords, batch):
    """host inputs: the span product the device would measure, before anything is copied"""
    span = 1
    for col in ([coords[:, a] for a in range(3)] + ([batch] if batch is not None else [])):
        span *= int(col.max()) - int(col.min()) + 1
    return span <= _SPAN_LIMIT


def _check_coords(coords, batch_index):
    """coords [V, 3] and batch_index [V] or None, int64 or int32, as given to a VoxelNeighbors or a SparseConvMap
    -> (coords, batch_index, V) as tensors where they are; nothing here needs a GPU"""
    coords, _ = as_tensor(coords, "coords")
    if coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError("coords must be a [V, 3] tensor of voxel coordinates")
    if coords.dtype not in (torch.int64, torch.int32):
        raise ValueError("coords must be int64 or int32, not %s" % coords.dtype)
    v = coords.shape[0]
    if batch_index is not None:
        batch_index, _ = as_tensor(batch_index, "batch_index")
        if batch_index.dim() != 1 or batch_index.shape[0] != v:
            raise ValueError("batch_index must be a [V] tensor, one value per row of coords")
        if batch_index.dtype not in (torch.int64, torch.int32):
            raise ValueError("batch_index must be int64 or int32, not %s" % batch_index.dtype)
    return coords, batch_index, v
