"""d3d_amd.voxel.sparse_conv -- strided sparse convolution and its inverse on the voxels: the layers that halve the grid between the
submanifold stages of a voxel backbone (SECOND, CenterPoint, PV-RCNN), and the ones a sparse U-Net comes back up with.  An extension
(the reference stops at the voxelizer).

    cmap = SparseConvMap(sp.coords, kernel_size=3, stride=2, padding=1)      # once per frame and layer
    y    = sparse_conv3d(vf, cmap, weight, bias)                 # [Vout, Cout], weight [27, C, Cout]
    nb2  = VoxelNeighbors(cmap.out_coords, batch_index=cmap.out_batch)       # the next stage's submanifold layers
    up   = sparse_inverse_conv3d(y2, cmap, weight_up)            # [V, C']: back on the ORIGINAL input sites

The relation between input and output rows is not symmetric, but it is a bijection between the entries of two tables
(table_out[r, k] == v <=> table_in[v, k] == r), so forward, backward and the inverse convolution are all plain gathers through one
of them and GEMMs: nothing is scattered, no float atomics of the library's own (kernels and the exact rules: csrc/vstride.hip,
include/d3d_hip.h; the gather is csrc/vnbr.hip's, the GEMMs are torch's).  method="fused" -- the only route of fp16 and bf16 -- runs
all of it on the MFMA kernels of csrc/vconv.hip instead, without the gathered buffer (see conv.subm_conv3d).

This module builds the map and its two views; the convolution through them is conv.py's (conv_front, TableConv, FusedTableConv):
sparse_conv3d reads `_down` and goes back through `_up`, sparse_inverse_conv3d the other way round.
"""
import ctypes
from math import gcd

import torch

from .. import _lib
from .._rows import ROW_MAX, device_of
from ._coords import _check_coords, _triple
from .conv import TableView, conv_front

_MAX_STEP = 2 ** 24
_OVERFLOW = "the spans of the output box (and batch values) multiply to more than 2^62"


def _i32x3(t):
    return (ctypes.c_int32 * 3)(*t)


def _fanout(ks, stride, dil):
    """P: the largest number of outputs one input can feed"""
    p = 1
    for k, s, d in zip(ks, stride, dil):
        p *= -(-k // (s // gcd(s, d)))
    return p


class SparseConvMap:
    """The output voxels of a strided sparse convolution over one frame's active voxels, and the two tables between them.

    :param coords: [V, 3] int64 (int32 is widened) voxel coordinates, any values (negative, offset); torch tensor (GPU or host) or
        numpy array.  (batch, coordinate) must be unique
    :param kernel_size: an int in 1 .. 7 (even sizes too), or three of them
    :param stride: an int >= 1, or three of them
    :param padding: an int >= 0, or three of them
    :param dilation: an int >= 1, or three of them
    :param batch_index: [V] int64 / int32 or None; voxels of different batch values never meet
    :param spatial_shape: (X, Y, Z) or None.  When given, outputs are kept only inside dense conv3d's output size
        floor((S + 2 p - d (k - 1) - 1) / s) + 1 per axis (ValueError if that is below 1), and an input outside [0, S) is refused
        (ValueError).  When None every output with a non-empty receptive field is active

    Input i feeds output o through column k = (ix * ky + iy) * kz + iz (VoxelNeighbors' order, the offsets uncentred) when
    o * stride - padding + (ix, iy, iz) * dilation == i on every axis (negative coordinates floor).  Output rows are numbered in the
    order of their first candidate (v, k), ascending in v * K + k: deterministic, a function of the input alone.

    Holds, on the GPU: `out_coords` [Vout, 3] int64, `out_batch` [Vout] int64 (None without a batch_index), `table_out` [Vout, K]
    int32 (the input row output r reads through column k) and `table_in` [V, K] int32 (table_in[v, k] == r <=> table_out[r, k] == v),
    -1 for none; and `num_voxels`, `num_out`, `num_entries` (the entries >= 0, the same number in both tables), `kernel_size`,
    `stride`, `padding`, `dilation`, `spatial_shape`, `kernel_volume`, `device`.  `out_coords` and `out_batch` feed the next stage's
    VoxelNeighbors(...) or SparseConvMap(...) directly.  Building it reads the device's counters back twice (the sizes before the
    outputs are allocated, the duplicate count after).  ValueError on duplicates, when the spans of the output box (and batch)
    multiply to more than 2^62 or the inputs span 2^62 or more on an axis, and when V * P > 2^31 - 1 (P: the product over the axes
    of ceil(k / (s / gcd(s, d))), the most outputs one input can feed)."""

    def __init__(self, coords, kernel_size, stride, padding=0, dilation=1, batch_index=None, spatial_shape=None):
        coords, batch_index, v = _check_coords(coords, batch_index)
        ks, st = _triple(kernel_size, "kernel_size"), _triple(stride, "stride")
        pad, dil = _triple(padding, "padding"), _triple(dilation, "dilation")
        if any(k < 1 or k > 7 for k in ks):
            raise ValueError("kernel_size must be in 1 .. 7, not %r" % (kernel_size,))
        if any(s < 1 or s > _MAX_STEP for s in st):
            raise ValueError("stride must be in 1 .. 2^24, not %r" % (stride,))
        if any(p < 0 or p > _MAX_STEP for p in pad):
            raise ValueError("padding must be in 0 .. 2^24, not %r" % (padding,))
        if any(d < 1 or d > _MAX_STEP for d in dil):
            raise ValueError("dilation must be in 1 .. 2^24, not %r" % (dilation,))
        shape = None
        if spatial_shape is not None:
            if isinstance(spatial_shape, (int, float)):
                raise ValueError("spatial_shape must be three ints, not %r" % (spatial_shape,))
            shape = _triple(spatial_shape, "spatial_shape")
            if any(s < 1 or s > ROW_MAX for s in shape):
                raise ValueError("spatial_shape must be in 1 .. 2^31 - 1 per axis, not %r" % (spatial_shape,))
            if any(s + 2 * p - d * (k - 1) - 1 < 0 for s, p, d, k in zip(shape, pad, dil, ks)):
                raise ValueError("a dense convolution of a %r grid with this kernel has no output" % (shape,))
        if v * _fanout(ks, st, dil) > ROW_MAX:
            raise ValueError("SparseConvMap takes at most 2^31 - 1 candidates V * P (P = %d here)" % _fanout(ks, st, dil))
        dev = device_of(coords)
        k = ks[0] * ks[1] * ks[2]
        self.device, self.num_voxels, self.kernel_volume = dev, v, k
        self.kernel_size, self.stride, self.padding, self.dilation, self.spatial_shape = ks, st, pad, dil, shape
        coords = coords.to(device=dev, dtype=torch.int64).contiguous()
        batch = None if batch_index is None else batch_index.to(device=dev, dtype=torch.int64).contiguous()
        vout = entries = dups = over = outside = 0
        with torch.cuda.device(dev):
            if v:
                lib = _lib.load()
                shape_arg = None if shape is None else (ctypes.c_int64 * 3)(*shape)
                args = (_lib.ptr(coords), _lib.ptr(batch), v, _i32x3(ks), _i32x3(st), _i32x3(pad), _i32x3(dil), shape_arg)
                counts = torch.empty((5,), dtype=torch.int64, device=dev)
                ws = _lib.workspace(lib.d3d_sparse_conv_map_workspace_bytes(v, _i32x3(ks), _i32x3(st), _i32x3(dil)), dev)
                rc = lib.d3d_sparse_conv_map_count(*args, _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
                _lib.check(rc, "sparse_conv_map_count")
                vout, entries, _, over, outside = counts.tolist()       # the sizes: only the device knows Vout
            if outside:
                raise ValueError("coords holds voxels outside spatial_shape %r" % (shape,))
            if over:
                raise ValueError(_OVERFLOW)
            self.out_coords = torch.empty((vout, 3), dtype=torch.int64, device=dev)
            self.out_batch = None if batch is None else torch.empty((vout,), dtype=torch.int64, device=dev)
            self.table_out = torch.empty((vout, k), dtype=torch.int32, device=dev)
            self.table_in = torch.empty((v, k), dtype=torch.int32, device=dev)
            if v:
                rc = lib.d3d_sparse_conv_map_emit(*args, vout, _lib.ptr(self.out_coords), _lib.ptr(self.out_batch), _lib.ptr(self.table_in),
                                                  _lib.ptr(self.table_out), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
                _lib.check(rc, "sparse_conv_map_emit")
                dups = int(counts[2])                                    # contested claims: two inputs on one (batch, coordinate)
        if dups:
            raise ValueError("coords holds rows whose (batch, coordinate) another row already has (%d contested table entries)" % dups)
        self.num_out, self.num_entries = vout, entries
        self._down = TableView(self.table_out, v, k, dev)               # output rows read input rows
        self._up = TableView(self.table_in, vout, k, dev)               # input rows read output rows


def sparse_conv3d(features, cmap, weight, bias=None, chunk_rows=None, method=None):
    """Strided sparse convolution: out[r] = sum over k of features[table_out[r, k]] @ weight[k] (+ bias), on the active outputs only.

    :param features: [V, Cin] float32, float64, float16 or bfloat16 (half precision: `method`), torch tensor (GPU or host) or numpy
        array; differentiable (once)
    :param cmap: the layer's SparseConvMap (its kernel size, stride, padding and dilation are the convolution's)
    :param weight: [K, Cin, Cout] in the dtype of features, K = cmap's kernel volume in the tables' column order (a dense conv3d
        weight [Cout, Cin, kx, ky, kz] is weight.permute(2, 3, 4, 1, 0).reshape(K, Cin, Cout), as for subm_conv3d); differentiable
    :param bias: [Cout] or None; differentiable
    :param chunk_rows: rows per gather step, as for subm_conv3d: every GEMM call has one fixed row count, so a row of the result and
        of grad_features does not depend on it
    :param method: "gather" (the default of float32 / float64) or "fused" (float32, float16, bfloat16; the default and the only route
        of the half types): as for subm_conv3d -- MFMA kernels, no gathered buffer, Cin and Cout multiples of 16 in 16 .. 256
    :return: [Vout, Cout] on the side features came from; row r belongs to cmap.out_coords[r].  It equals dense conv3d at the
        active outputs.  Gradients: grad_features[v] = sum_k grad_out[table_in[v, k]] @ weight[k]^T (a gather through table_in, no
        mirroring), grad_weight = the sum over the chunks, in chunk order, of gathered^T @ grad_out, grad_bias = the column sum
    """
    if not isinstance(cmap, SparseConvMap):
        raise TypeError("cmap must be a SparseConvMap")
    return conv_front(features, cmap, cmap._down, cmap._up, False, weight, bias, chunk_rows, method)


def sparse_inverse_conv3d(features, cmap, weight, bias=None, chunk_rows=None, method=None):
    """Inverse sparse convolution (spconv's SparseInverseConv3d): out[v] = sum over k of features[table_in[v, k]] @ weight[k]
    (+ bias) -- conv_transpose3d of the output-side rows, evaluated on the ORIGINAL input sites of `cmap`.

    :param features: [Vout, Cin] float32, float64, float16 or bfloat16 (half precision: `method`), one row per cmap.out_coords; torch
        tensor (GPU or host) or numpy array; differentiable (once)
    :param cmap: the SparseConvMap of the strided layer this one undoes
    :param weight: [K, Cin, Cout] in the tables' column order (a conv_transpose3d weight [Cin, Cout, kx, ky, kz] is
        weight.permute(2, 3, 4, 0, 1).reshape(K, Cin, Cout)); differentiable
    :param bias, chunk_rows, method: as for sparse_conv3d
    :return: [V, Cout] on the side features came from; row v belongs to the coords[v] cmap was built from.  Its backward runs
        through table_out the same way
    """
    if not isinstance(cmap, SparseConvMap):
        raise TypeError("cmap must be a SparseConvMap")
    return conv_front(features, cmap, cmap._up, cmap._down, False, weight, bias, chunk_rows, method)


__all__ = ["SparseConvMap", "sparse_conv3d", "sparse_inverse_conv3d"]
