"""The numpy model of d3d_table_pool_forward / d3d_table_pool_backward (csrc/vtpool.hip; d3d_amd.voxel.sparse_pool), written from the
rules of include/d3d_hip.h and from nothing else: one pass over the columns of the table in ascending order, every row at once.

The arithmetic is the kernel's: fp64 in np.float64, fp32 in np.float32; the half types fold in np.float32 (their values are fp32
values) and are rounded once by table_conv_reference.round_to.  Features and gradients come and go as numpy arrays in the FOLD type
(float64 for "f64", float32 otherwise) that hold values of the kind exactly; `to_tensor` makes the tensor of the kind of a result."""
import numpy as np
import torch

import table_conv_reference as tref

SUM, MEAN, MAX, MIN = "sum", "mean", "max", "min"
REDUCTIONS = (SUM, MEAN, MAX, MIN)
KINDS = ("f32", "f64", "f16", "bf16")
TORCH = dict(tref.TORCH, f64=torch.float64)
CODES = {"f32": 0, "f64": 1, "f16": 4, "bf16": 5}               # D3D_F32, D3D_F64, D3D_F16, D3D_BF16
RED_CODES = {MEAN: 1, MAX: 2, MIN: 3, SUM: 4}                    # D3D_REDUCE_*, SUM = 4


def fold_type(kind):
    return np.float64 if kind == "f64" else np.float32


def of_kind(x, kind):
    """any float array -> (a CPU tensor of `kind`, rounded to it, and the same values as an array of the fold type)"""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(TORCH[kind])
    return t, t.to(torch.float64 if kind == "f64" else torch.float32).numpy()


def to_tensor(x, kind):
    """a result in the fold type -> the CPU tensor of `kind` the kernel stores: one rounding to nearest even for the half types
    (NaN stays NaN: round_to takes finite values and infinities only)"""
    if kind == "f64":
        return torch.from_numpy(np.ascontiguousarray(x, np.float64).copy())
    x = np.ascontiguousarray(x, np.float32)
    nan = np.isnan(x)
    t = tref.round_to(np.where(nan, np.float32(0), x), kind)
    t[torch.from_numpy(nan)] = float("nan")
    return t


def forward(feat, table, reduction, kind):
    """feat [S, C] in the fold type, table [R, K] with entries in [-1, S) -> (out [R, C] in the fold type, before the final rounding;
    arg [R, C] int16, the winning column of max / min, -1 without one (all -1 for sum / mean); count [R] int32).
    sum: 0 + x_0 + x_1 + ... over the present entries in ascending column; mean: that sum / (T)count, one division; max / min: the
    first x > best (x < best) wins, NaN wins over every number and the first NaN stays, -0.0 == +0.0; a row without entries: 0"""
    d = fold_type(kind)
    feat = np.asarray(feat)
    assert feat.dtype == d and reduction in REDUCTIONS
    r, k = table.shape
    c = feat.shape[1]
    acc, win, n = np.zeros((r, c), d), np.full((r, c), -1, np.int16), np.zeros(r, np.int32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for kk in range(k):
            e = table[:, kk].astype(np.int64)
            here = (e >= 0)[:, None]
            if not here.any():
                continue
            x = feat[np.maximum(e, 0)] if len(feat) else np.zeros((r, c), d)
            if reduction in (SUM, MEAN):
                acc = np.where(here, acc + x, acc)
            else:
                better = (x > acc) if reduction == MAX else (x < acc)
                take = here & ((win < 0) | (~np.isnan(acc) & (better | np.isnan(x))))
                acc, win = np.where(take, x, acc), np.where(take, np.int16(kk), win)
            n += here[:, 0]
        if reduction == MEAN:
            acc = np.where((n > 0)[:, None], acc / np.maximum(n, 1).astype(d)[:, None], acc)
    assert acc.dtype == d
    return acc, win, n


def backward(grad, back_table, mirrored, reduction, kind, arg=None, count=None):
    """grad [Rout, C] in the fold type, back_table [V, K] with entries in [-1, Rout), arg / count as `forward` returned them ->
    grad_feat [V, C] in the fold type, before the final rounding: 0 + the contributions of the present entries in ascending column kk
    -- grad[e] (sum), grad[e] / (T)count[e] (mean), grad[e, ch] where arg[e, ch] == (K - 1 - kk if mirrored else kk) (max / min)"""
    d = fold_type(kind)
    grad = np.asarray(grad)
    assert grad.dtype == d and reduction in REDUCTIONS
    v, k = back_table.shape
    c = grad.shape[1]
    acc = np.zeros((v, c), d)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for kk in range(k):
            e = back_table[:, kk].astype(np.int64)
            here = (e >= 0)[:, None]
            if not here.any():
                continue
            ee = np.maximum(e, 0)
            g = grad[ee]
            if reduction == MEAN:
                g = g / count[ee].astype(d)[:, None]
            elif reduction in (MAX, MIN):
                here = here & (arg[ee] == (k - 1 - kk if mirrored else kk))
            acc = np.where(here, acc + g, acc)
    assert acc.dtype == d
    return acc


def brute(feat, coords, batch, out_coords, out_batch, kernel_size, stride, padding, dilation, reduction):
    """the forward from the coordinates alone, in fp64 and with no table: output o reduces every input i with
    i == o * stride - padding + (ix, iy, iz) * dilation for a column (ix, iy, iz) inside the kernel, taken in ascending column
    -> (out [Rout, C] float64, count [Rout]); max / min by np.max / np.min (no NaN, no ties to break)"""
    ks, st, pad, dil = (np.array(x, np.int64) for x in (kernel_size, stride, padding, dilation))
    out, count = np.zeros((len(out_coords), feat.shape[1])), np.zeros(len(out_coords), np.int32)
    for r, (o, ob) in enumerate(zip(out_coords, out_batch)):
        diff = coords - (o * st - pad)
        step = diff // dil
        hit = np.all((diff % dil == 0) & (step >= 0) & (step < ks), 1) & (batch == ob)
        rows = np.nonzero(hit)[0]
        rows = rows[np.argsort((step[rows, 0] * ks[1] + step[rows, 1]) * ks[2] + step[rows, 2])]
        count[r] = len(rows)
        if len(rows):
            x = feat[rows].astype(np.float64)
            out[r] = {SUM: x.sum(0), MEAN: x.mean(0), MAX: x.max(0), MIN: x.min(0)}[reduction]
    return out, count


def canonical_nan(t):
    """a float tensor with every NaN replaced by one NaN: the rules say WHERE a NaN is, not which payload it carries"""
    t = t.detach().cpu().clone()
    t[torch.isnan(t)] = float("nan")
    return t


def equal_bits(got, want):
    """same shape, dtype and bits, a NaN equal to any NaN"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == torch.float64:
        a, b = canonical_nan(got).view(torch.int64).numpy(), canonical_nan(want).view(torch.int64).numpy()
        return np.array_equal(a, b)
    return tref.equal_bits(canonical_nan(got), canonical_nan(want))
