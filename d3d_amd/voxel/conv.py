"""d3d_amd.voxel.conv -- submanifold sparse convolution on the voxelizer's output: the neighbour table of the active voxels, the
gather of the neighbours' rows and the convolution built from them, all differentiable: what every voxel backbone (SECOND,
CenterPoint, PV-RCNN, sparse U-Nets) opens with.  An extension (the reference stops at the voxelizer).

    sp   = VoxelGenerator(bounds, shape, max_points=32, max_points_filter="trim")(pts)    # sparse contract
    vf   = voxel_pool(mlp(sp.points), VoxelIndex(sp.points_mapping, len(sp.coords)))     # [V, C]
    nbrs = VoxelNeighbors(sp.coords, kernel_size=3)              # once per frame; every layer and every backward reuses it
    y    = subm_conv3d(vf, nbrs, weight, bias)                   # [V, Cout], weight [27, C, Cout]

The neighbour relation is symmetric (table[v, k] == u <=> table[u, K-1-k] == v), so the gradient of a gather through the table is
the gather through the mirrored columns: forward and backward are gathers and GEMMs, nothing is scattered, no float atomics of the
library's own (kernels and the exact rules: csrc/vnbr.hip, include/d3d_hip.h; the GEMMs are torch's).

    y    = subm_conv3d(vf.bfloat16(), nbrs, weight.bfloat16(), method="fused")      # fp32 / fp16 / bf16 on the matrix cores

method="fused" (the only route of fp16 and bf16) runs the convolution and its gradients as MFMA kernels that gather the rows straight
into LDS: no [V, K * C] buffer exists (csrc/vconv.hip).

Everything that convolves through a table lives here, once, for subm_conv3d and for sparse_conv.py's two operators: a TableView per
table, conv_front (the argument checks and the choice of the route), and one autograd.Function per route, TableConv (gather) and
FusedTableConv, over a forward and a backward view: out[r] = sum_k features[fwd.table[r, k]] @ weight[k] (+ bias).
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._rows import FEATURE_CODES, FLOAT_CODES, ROW_MAX, as_tensor, back_to_caller, check_rows, device_of, dtype_code, on_owner, to_owner
from ._coords import _check_coords, _host_spans_fit, _triple

_GATHER_BYTES = 1 << 30           # what the default chunk_rows lets one gathered buffer take
_GEMM_TILE_BYTES = 1 << 28        # the gathered rows of one GEMM call
_GEMM_TILE_ROWS = (1024, 65536)


class TableView:
    """what the gathers, the fused launchers and _chunk_rows read of a table [num_voxels, K] whose entries point into src_rows feature
    rows: the one table of a VoxelNeighbors (src_rows = num_voxels), the two of a SparseConvMap"""

    def __init__(self, table, src_rows, kernel_volume, device):
        self.table, self.num_voxels, self.src_rows, self.kernel_volume, self.device = table, table.shape[0], src_rows, kernel_volume, device


class VoxelNeighbors:
    """The neighbour table of one frame's active voxels.

    :param coords: [V, 3] int64 (int32 is widened) voxel coordinates, any values (negative, offset); torch tensor (GPU or host)
        or numpy array.  (batch, coordinate) must be unique
    :param kernel_size: an odd int in 1 .. 7, or three of them
    :param dilation: an int >= 1, or three of them
    :param batch_index: [V] int64 / int32 or None; voxels of different batch values are never neighbours

    Holds `table` [V, K] int32 on the GPU, K = kx * ky * kz: column k = (ix * ky + iy) * kz + iz is the row of the voxel at
    coords[v] + ((ix, iy, iz) - (k* - 1) / 2) * dilation, -1 where there is none; `kernel_size`, `dilation`, `num_voxels` and
    `num_entries` (the entries >= 0).  Building it reads three numbers back, once.  ValueError on duplicates and when the product
    of the coordinate (and batch) spans exceeds 2^62."""

    def __init__(self, coords, kernel_size=3, dilation=1, batch_index=None):
        coords, batch_index, v = _check_coords(coords, batch_index)
        ks, dil = _triple(kernel_size, "kernel_size"), _triple(dilation, "dilation")
        if any(k < 1 or k > 7 or k % 2 == 0 for k in ks):
            raise ValueError("kernel_size must be odd and in 1 .. 7, not %r" % (kernel_size,))
        if any(d < 1 or d >= 2 ** 31 for d in dil):
            raise ValueError("dilation must be at least 1, not %r" % (dilation,))
        if v > ROW_MAX:
            raise ValueError("VoxelNeighbors takes at most 2^31 - 1 voxels")
        overflow = "the spans of the coordinates (and batch values) multiply to more than 2^62"
        if v and not coords.is_cuda and not _host_spans_fit(coords, None if batch_index is None or batch_index.is_cuda else batch_index):
            raise ValueError(overflow)
        dev = device_of(coords)
        k = ks[0] * ks[1] * ks[2]
        self.device, self.num_voxels, self.kernel_size, self.dilation, self.kernel_volume = dev, v, ks, dil, k
        coords = coords.to(device=dev, dtype=torch.int64).contiguous()
        batch = None if batch_index is None else batch_index.to(device=dev, dtype=torch.int64).contiguous()
        with torch.cuda.device(dev):
            self.table = torch.empty((v, k), dtype=torch.int32, device=dev)
            entries = dups = over = 0
            if v:
                lib = _lib.load()
                counts = torch.empty((3,), dtype=torch.int64, device=dev)
                ws = _lib.workspace(lib.d3d_voxel_neighbors_workspace_bytes(v), dev)
                rc = lib.d3d_voxel_neighbors(_lib.ptr(coords), _lib.ptr(batch), v, ks[0], ks[1], ks[2], dil[0], dil[1], dil[2],
                                             _lib.ptr(self.table), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
                _lib.check(rc, "voxel_neighbors")
                entries, dups, over = counts.tolist()            # the one read-back of a frame's table
        if over:
            raise ValueError(overflow)
        if dups:
            raise ValueError("coords holds %d rows whose (batch, coordinate) an earlier row already has" % dups)
        self.num_entries = entries
        self._view = TableView(self.table, v, k, dev)           # the voxels read the voxels: forward as it is, backward mirrored


def _gather(feat, nbrs, mirrored, v0=0, rows=None, feat_cols=1, out=None):
    """feat [V, C] (or [V, K, C] with feat_cols = K) on nbrs.device -> [rows, K, C] for the rows v0 .. v0 + rows of the table (into
    `out`, contiguous and of that many elements, when given); one launch, every output row written once.  nbrs: a TableView
    (V = nbrs.src_rows, the table has nbrs.num_voxels rows)"""
    k, c = nbrs.kernel_volume, feat.shape[-1]
    rows = nbrs.num_voxels - v0 if rows is None else rows
    with torch.cuda.device(nbrs.device):
        if rows == 0 or c == 0:
            return feat.new_zeros((rows, k, c)) if out is None else out
        if out is None:
            out = torch.empty((rows, k, c), dtype=feat.dtype, device=nbrs.device)
        code = dtype_code(feat, FLOAT_CODES, "voxel features")
        rc = _lib.load().d3d_neighbor_gather(_lib.ptr(feat), nbrs.src_rows, c, code, feat_cols, _lib.ptr(nbrs.table[v0:]),
                                             rows, k, int(mirrored), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "neighbor_gather")
    return out


def _gather_sum(grad, nbrs):
    """grad [V, K, C] on nbrs.device -> [V, C]: the mirrored gather of it (row [table[u, K-1-k], k] for every (u, k)), then the sum
    over k in ascending k"""
    g = _gather(grad, nbrs, True, feat_cols=nbrs.kernel_volume)
    acc = g[:, 0].clone()
    for k in range(1, nbrs.kernel_volume):                       # a fixed left fold: the same bits on every run
        acc += g[:, k]
    return acc


class NeighborGather(torch.autograd.Function):
    """neighbor_gather: (features [V, C], the view of a VoxelNeighbors) -> [V, K, C], one launch.  backward: the mirrored gather of
    the gradient, summed over k (_gather_sum).  Differentiable once."""

    @staticmethod
    def forward(ctx, features, nbrs):
        ctx.nbrs, ctx.odev = nbrs, features.device
        return on_owner(_gather, features, nbrs, ctx.odev, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        return on_owner(_gather_sum, grad, ctx.nbrs, ctx.odev), None


def _chunks(v, chunk_rows):
    return [(v0, min(chunk_rows, v - v0)) for v0 in range(0, v, chunk_rows)]


def _gemm_rows(row_bytes, v):
    """the rows of every GEMM call for gathered rows of `row_bytes` on a frame of v voxels: a power of two that keeps a call's
    gathered rows at about 256 MiB, between 1024 and 65536, and no more than the power of two that covers the frame.  It depends on
    the row and on V -- not on chunk_rows"""
    g = _GEMM_TILE_ROWS[0]
    while g < _GEMM_TILE_ROWS[1] and 2 * g * max(row_bytes, 1) <= _GEMM_TILE_BYTES:
        g *= 2
    while g > 1 and g // 2 >= v:
        g //= 2
    return g


def _gather_times(feat, nbrs, mirrored, v0, r, mat, out):
    """out[v0 : v0 + r] = (the gathered rows [r, K * C] of the table's rows v0 .. v0 + r) @ mat.
    Every GEMM call has exactly _gemm_rows(..) rows, the last one of the frame padded with zero rows: torch.matmul picks its kernel,
    and with it the order of a row's additions, by the shape of the call.  Measured on an MI355X: the same rows differ in the last
    bits between calls of 4097 and of 1000 rows, in fp32 and fp64, while inside calls of one shape a row's bits depended neither on
    its position nor on the other rows (an observation about torch's GEMM, not a guarantee of it).  With one shape for every call a
    row's result does not depend on chunk_rows."""
    kc = nbrs.kernel_volume * feat.shape[1]
    tile = _gemm_rows(kc * feat.element_size(), nbrs.num_voxels)
    padded = -(-r // tile) * tile
    buf = torch.empty((padded, kc), dtype=feat.dtype, device=nbrs.device)
    _gather(feat, nbrs, mirrored, v0, r, out=buf[:r])
    buf[r:].zero_()
    for t0 in range(0, r, tile):
        n = min(tile, r - t0)
        out[v0 + t0:v0 + t0 + n] = torch.matmul(buf[t0:t0 + tile], mat)[:n]


def _chunk_rows(chunk_rows, nbrs, cin, cout, itemsize):
    """the rows per gather step: what the caller asked for (default: a gathered buffer of about 1 GiB), rounded UP to whole GEMM
    calls of the wider of the two gathers -- a buffer holds at least one call's rows anyway, so a smaller step would only pad every
    step to that size and multiply zero rows"""
    k = nbrs.kernel_volume
    if chunk_rows is None:
        chunk_rows = max(1, _GATHER_BYTES // (k * max(cin, cout, 1) * itemsize))
    tile = max(_gemm_rows(k * cin * itemsize, nbrs.num_voxels), _gemm_rows(k * cout * itemsize, nbrs.num_voxels))
    return -(-chunk_rows // tile) * tile


def _conv_enter(ctx, features, fwd, bwd, bwd_mirrored, weight, bias):
    """what both routes' forward begins with: -> (features, weight, bias or None) detached, contiguous and on the tables' device;
    on ctx the two views, the two of them saved, and the device each of the three came from"""
    f, w = to_owner(features, fwd), to_owner(weight, fwd)
    b = None if bias is None else to_owner(bias, fwd)
    ctx.fwd, ctx.bwd, ctx.bwd_mirrored = fwd, bwd, bwd_mirrored
    ctx.devs = (features.device, weight.device, None if bias is None else bias.device)
    ctx.save_for_backward(f, w)
    return f, w, b


def _conv_grads(ctx, gf, gw, gb):
    """what both routes' backward ends with: the gradients that were asked for (None: not), each on its caller's device, in the
    places of (features, fwd, bwd, bwd_mirrored, weight, bias)"""
    gf, gw, gb = (None if g is None else _lib.to_caller(g, odev, ctx.fwd.device) for g, odev in zip((gf, gw, gb), ctx.devs))
    return gf, None, None, None, gw, gb


class TableConv(torch.autograd.Function):
    """The gather route of all three operators: out[r] = sum_k features[fwd.table[r, k]] @ weight[k] (+ bias) for two views that are
    each other's transposed map: subm_conv3d passes a VoxelNeighbors' one view twice and reads it mirrored on the way back
    (table[v, k] == u <=> table[u, K-1-k] == v), the operators of a SparseConvMap its two views, unmirrored (fwd.table[r, k] == v <=>
    bwd.table[v, k] == r).  Per chunk of rows one gather [R, K * Cin] and GEMMs of a fixed row count with weight [K * Cin, Cout]
    (_gather_times).  backward: grad_features = the gather of grad_out through bwd.table [R', K * Cout] times weight^T [K * Cout,
    Cin]; grad_weight = the sum over the chunks of fwd, in chunk order, of gathered^T @ grad_out (the gather is made again, not
    kept); grad_bias = the column sum.  Differentiable once."""

    @staticmethod
    def forward(ctx, features, fwd, bwd, bwd_mirrored, weight, bias, chunk_fwd, chunk_bwd):
        f, w, b = _conv_enter(ctx, features, fwd, bwd, bwd_mirrored, weight, bias)
        k, cin, cout = w.shape
        ctx.chunks = (chunk_fwd, chunk_bwd)
        with torch.cuda.device(fwd.device):
            out = torch.empty((fwd.num_voxels, cout), dtype=f.dtype, device=fwd.device)
            for r0, r in _chunks(fwd.num_voxels, chunk_fwd):
                _gather_times(f, fwd, False, r0, r, w.view(k * cin, cout), out)
            if b is not None:
                out += b
        return _lib.to_caller(out, features.device, fwd.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        f, w = ctx.saved_tensors
        fwd, bwd = ctx.fwd, ctx.bwd
        k, cin, cout = w.shape
        g = to_owner(grad, fwd)
        need_f, _, _, _, need_w, need_b, _, _ = ctx.needs_input_grad
        gf = gw = gb = None
        with torch.cuda.device(fwd.device):
            if need_f:
                gf = torch.empty_like(f)
                wt = w.transpose(1, 2).reshape(k * cout, cin)
                for v0, r in _chunks(bwd.num_voxels, ctx.chunks[1]):
                    _gather_times(g, bwd, ctx.bwd_mirrored, v0, r, wt, gf)
            if need_w:
                gw = torch.zeros((k * cin, cout), dtype=w.dtype, device=fwd.device)
                for r0, r in _chunks(fwd.num_voxels, ctx.chunks[0]):
                    gw += torch.matmul(_gather(f, fwd, False, r0, r).view(r, k * cin).t(), g[r0:r0 + r])
                gw = gw.view(k, cin, cout)
            if need_b:
                gb = g.sum(0)
        return _conv_grads(ctx, gf, gw, gb) + (None, None)


_FUSED_CODES = {d: code for d, code in FEATURE_CODES.items() if d != torch.float64}
_METHODS = (None, "gather", "fused")


def _conv_dtype(t):
    """the dtypes a convolution takes (neighbor_gather and voxel_pool keep to float32 and float64)"""
    dtype_code(t, FEATURE_CODES, "voxel features")


def _conv_route(features, weight, method):
    """"gather" or "fused" for features [*, Cin] and weight [K, Cin, Cout] of one dtype: fp32 / fp64 take the gather route unless
    asked, half precision exists on the fused kernels only; ValueError for what the chosen route does not serve"""
    if method not in _METHODS:
        raise ValueError("method must be None, \"gather\" or \"fused\", not %r" % (method,))
    if features.dtype in (torch.float16, torch.bfloat16):
        if method == "gather":
            raise ValueError("%s runs on the fused kernels only: method=\"gather\" takes float32 and float64" % features.dtype)
        method = "fused"
    if method != "fused":
        return "gather"
    if features.dtype == torch.float64:
        raise ValueError("method=\"fused\" takes float32, float16 and bfloat16, not float64")
    for c, what in ((weight.shape[1], "Cin"), (weight.shape[2], "Cout")):
        if c < 16 or c > 256 or c % 16:
            raise ValueError("the fused kernels take channel counts that are multiples of 16 in 16 .. 256, not %s = %d" % (what, c))
    return "fused"


def _table_conv(feat, view, mirrored, weight, bias):
    """d3d_table_conv: out[r] = bias + sum_k feat[view.table[r, mirrored ? K - 1 - k : k]] @ weight[k], one launch, no workspace"""
    k, cin, cout = weight.shape
    with torch.cuda.device(view.device):
        out = torch.empty((view.num_voxels, cout), dtype=feat.dtype, device=view.device)
        rc = _lib.load().d3d_table_conv(_lib.ptr(feat), view.src_rows, cin, _lib.ptr(view.table), view.num_voxels, k, int(mirrored),
                                        _lib.ptr(weight), _lib.ptr(bias), cout, _FUSED_CODES[feat.dtype], _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "table_conv")
    return out


def _table_conv_wgrad(feat, view, mirrored, grad, k):
    """d3d_table_conv_wgrad: grad_weight[k] = sum_r feat[view.table[r, k]]^T (x) grad[r], fp32 partials per row slab folded in order"""
    cin, cout, rows = feat.shape[1], grad.shape[1], view.num_voxels
    with torch.cuda.device(view.device):
        lib = _lib.load()
        gw = torch.empty((k, cin, cout), dtype=feat.dtype, device=view.device)
        ws = _lib.workspace(lib.d3d_table_conv_wgrad_workspace_bytes(rows, k, cin, cout), view.device)
        rc = lib.d3d_table_conv_wgrad(_lib.ptr(feat), view.src_rows, cin, _lib.ptr(view.table), rows, k, int(mirrored), _lib.ptr(grad), cout,
                                      _FUSED_CODES[feat.dtype], _lib.ptr(gw), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "table_conv_wgrad")
    return gw


class FusedTableConv(torch.autograd.Function):
    """The fused route of all three operators: TableConv's result from the same two views on the MFMA kernels of csrc/vconv.hip,
    without chunks, the bias added inside the kernel.  backward: grad_features = d3d_table_conv of grad_out through bwd with weight
    transposed to [K, Cout, Cin]; grad_weight = d3d_table_conv_wgrad through fwd; grad_bias = the column sum, accumulated in fp32.
    Everything comes back in the dtype of features.  Differentiable once."""

    @staticmethod
    def forward(ctx, features, fwd, bwd, bwd_mirrored, weight, bias):
        f, w, b = _conv_enter(ctx, features, fwd, bwd, bwd_mirrored, weight, bias)
        return _lib.to_caller(_table_conv(f, fwd, False, w, b), features.device, fwd.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        f, w = ctx.saved_tensors
        g = to_owner(grad, ctx.fwd)
        need_f, _, _, _, need_w, need_b = ctx.needs_input_grad
        gf = gw = gb = None
        with torch.cuda.device(ctx.fwd.device):
            if need_f:
                gf = _table_conv(g, ctx.bwd, ctx.bwd_mirrored, w.transpose(1, 2).contiguous(), None)
            if need_w:
                gw = _table_conv_wgrad(f, ctx.fwd, False, g, w.shape[0])
            if need_b:
                gb = g.sum(0, dtype=torch.float32).to(g.dtype)
        return _conv_grads(ctx, gf, gw, gb)


def conv_front(features, owner, fwd, bwd, bwd_mirrored, weight, bias, chunk_rows, method):
    """What subm_conv3d, sparse_conv3d and sparse_inverse_conv3d do once each has checked its owner's type and picked the forward and
    the backward view of it: numpy in and out, every check of the arguments (shapes first, then what the route refuses), the route,
    the chunk sizes of the gather route, and the call of that route's Function"""
    features, was_numpy = as_tensor(features, "features")
    weight, _ = as_tensor(weight, "weight")
    check_rows(features, "features", "voxel", "voxel features", FEATURE_CODES, owner, fwd.src_rows)
    if weight.dim() != 3 or weight.shape[0] != fwd.kernel_volume or weight.shape[1] != features.shape[1]:
        raise ValueError("weight must be [K, Cin, Cout] = [%d, %d, Cout], not %s" % (fwd.kernel_volume, features.shape[1], tuple(weight.shape)))
    if weight.dtype != features.dtype:
        raise ValueError("weight is %s, features %s" % (weight.dtype, features.dtype))
    cin, cout, size = weight.shape[1], weight.shape[2], features.element_size()
    if bias is not None:
        bias, _ = as_tensor(bias, "bias")
        if bias.dim() != 1 or bias.shape[0] != cout or bias.dtype != features.dtype:
            raise ValueError("bias must be [Cout] = [%d] in %s, the dtype of features" % (cout, features.dtype))
    if chunk_rows is not None:
        chunk_rows = int(chunk_rows)
        if chunk_rows < 1:
            raise ValueError("chunk_rows must be at least 1, not %d" % chunk_rows)
    if _conv_route(features, weight, method) == "fused":
        out = FusedTableConv.apply(features, fwd, bwd, bwd_mirrored, weight, bias)
    else:
        out = TableConv.apply(features, fwd, bwd, bwd_mirrored, weight, bias, _chunk_rows(chunk_rows, fwd, cin, cout, size),
                              _chunk_rows(chunk_rows, bwd, cin, cout, size))
    return back_to_caller(out, was_numpy)


def neighbor_gather(features, nbrs):
    """The rows of every voxel's neighbours, side by side.

    :param features: [V, C] float32 or float64, torch tensor (GPU or host) or numpy array; differentiable (once)
    :param nbrs: the frame's VoxelNeighbors
    :return: [V, K, C] on the caller's side: row [v, k] = features[table[v, k]], zero where table[v, k] == -1.  Its gradient is
        grad_features[u] = grad[table[u, K-1], 0] + grad[table[u, K-2], 1] + ... in that order (absent neighbours add +0)
    """
    if not isinstance(nbrs, VoxelNeighbors):
        raise TypeError("nbrs must be a VoxelNeighbors")
    features, was_numpy = as_tensor(features, "features")
    check_rows(features, "features", "voxel", "voxel features", FLOAT_CODES, nbrs, nbrs.num_voxels)
    out = NeighborGather.apply(features, nbrs._view)
    return back_to_caller(out, was_numpy)


def subm_conv3d(features, nbrs, weight, bias=None, chunk_rows=None, method=None):
    """Submanifold sparse convolution: out[v] = sum over k of features[table[v, k]] @ weight[k] (+ bias), on the active voxels only.

    :param features: [V, Cin] float32, float64, float16 or bfloat16 (half precision: `method`), torch tensor (GPU or host) or numpy
        array; differentiable (once)
    :param nbrs: the frame's VoxelNeighbors (its kernel size and dilation are the convolution's)
    :param weight: [K, Cin, Cout] in the dtype of features, K = nbrs' kernel volume in the table's column order (a dense
        conv3d weight [Cout, Cin, kx, ky, kz] is weight.permute(2, 3, 4, 1, 0).reshape(K, Cin, Cout)); differentiable
    :param bias: [Cout] or None; differentiable
    :param chunk_rows: voxels per gather step, rounded up to whole GEMM calls; the default keeps one gathered buffer at about 1 GiB.
        Every GEMM call has the same row count (min(65536, a power of two covering V), fewer for rows beyond 4 KiB: about 256 MiB
        of gathered rows at most), the last call of the frame padded with zero rows, so that a row of the result and of
        grad_features does not depend on chunk_rows (measured, see _gather_times); a gathered buffer is at least one call's rows
    :param method: "gather" (the default of float32 / float64, what is described above), or "fused" (float32, float16, bfloat16; the
        default and the only route of the half types): the MFMA kernels of csrc/vconv.hip, which gather the rows straight into LDS --
        no [V, K * C] buffer, chunk_rows is checked and ignored.  Cin and Cout must be multiples of 16 in 16 .. 256 (ValueError).
        Products accumulate in fp32, the result is rounded once; outputs and all three gradients come back in the dtype of features,
        a row's bits depend on that row's neighbours alone, and every run gives the same bits
    :return: [V, Cout] on the side features came from
    """
    if not isinstance(nbrs, VoxelNeighbors):
        raise TypeError("nbrs must be a VoxelNeighbors")
    return conv_front(features, nbrs, nbrs._view, nbrs._view, True, weight, bias, chunk_rows, method)


__all__ = ["VoxelNeighbors", "neighbor_gather", "subm_conv3d", "NeighborGather", "TableConv", "FusedTableConv"]
