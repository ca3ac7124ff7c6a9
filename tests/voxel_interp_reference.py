"""The numpy model of d3d_voxel_corners, d3d_table_interp_forward and d3d_table_interp_backward (csrc/vnbr.hip, csrc/vinterp.hip;
d3d_amd.voxel.interp), written from the rules of include/d3d_hip.h and from nothing else.

The arithmetic is the kernels': positions and weights in the dtype of the positions (np.float32 / np.float64 arrays, one ufunc per
operation, so nothing contracts); features in np.float64 for "f64" and in np.float32 otherwise -- the half types multiply and add in
np.float32 (their values are fp32 values) and are rounded once by sparse_pool_reference.to_tensor.  Features and gradients come and go
as numpy arrays in the FOLD type, as in sparse_pool_reference."""
import numpy as np

import sparse_pool_reference as pref

KINDS = pref.KINDS
CODES = pref.CODES
MODES = {"linear": 8, "nearest": 1}
LIMIT = 2.0 ** 62
fold_type, of_kind, to_tensor, equal_bits = pref.fold_type, pref.of_kind, pref.to_tensor, pref.equal_bits


def _batch(n, batch):
    return np.zeros(n, np.int64) if batch is None else np.asarray(batch, np.int64)


def base(positions, mode):
    """positions [K, 3] fp32 / fp64 -> (ok [K]: finite and in [-2^62, 2^62) on every axis; b [K, 3] int64, the first corner (zero
    where not ok); f [K, 3] in the dtype, the fraction).  linear: b = floor(x), f = x - b, one operation each; nearest: b = floor(x + 0.5)"""
    x = np.asarray(positions)
    d = x.dtype.type
    assert x.dtype in (np.float32, np.float64) and x.ndim == 2 and x.shape[1] == 3
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.all(np.isfinite(x) & (x >= d(-LIMIT)) & (x < d(LIMIT)), 1)
        safe = np.where(ok[:, None], x, d(0))
        if mode == "nearest":
            b = np.floor(safe + d(0.5))
            f = np.zeros_like(safe)
        else:
            b = np.floor(safe)
            f = safe - b
    assert b.dtype == x.dtype and f.dtype == x.dtype
    return ok, b.astype(np.int64), f


def corners(coords, positions, batch=None, position_batch=None, mode="linear", normalize=False):
    """-> (table [K, J] int32, weights [K, J] in the dtype of positions), J = 8 (linear) or 1 (nearest).
    Corner j = dx * 4 + dy * 2 + dz is the voxel at b + (dx, dy, dz) with the point's batch value; -1 and weight 0 where there is none.
    A corner outside the box of the coordinates (and batch values) is absent before any look-up, as on the device; inside it the
    mixed-radix key over the spans is looked up among the sorted keys of the voxels.
    w_j = (wx * wy) * wz, wa = f_a where the corner's bit on axis a is set, else 1 - f_a.  normalize: s = 0 + w_j0 + w_j1 + ... over the
    present corners in ascending j, every present weight w_j / s; all 0 where no corner is present or s == 0"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    x = np.asarray(positions)
    d = x.dtype.type
    k, v, jn = len(x), len(c), MODES[mode]
    assert (batch is None) == (position_batch is None)
    ok, b, f = base(x, mode)
    table, w = np.full((k, jn), -1, np.int32), np.zeros((k, jn), x.dtype)
    if v and k:
        cb, pb = _batch(v, batch), _batch(k, position_batch)
        full = np.concatenate([cb[:, None], c], 1)                       # (batch, x, y, z): the key's digits, most significant first
        lo, hi = full.min(0), full.max(0)
        span = [int(h) - int(l) + 1 for l, h in zip(lo, hi)]
        assert span[0] * span[1] * span[2] * span[3] <= 2 ** 62

        def keys(rows, inside):
            key = np.zeros(len(rows), np.int64)
            for a in range(4):
                key = key * span[a] + (np.where(inside, rows[:, a], lo[a]) - lo[a])
            return key
        vkeys = keys(full, np.ones(v, bool))
        by_key = np.argsort(vkeys, kind="stable")
        sorted_keys = vkeys[by_key]
        assert np.all(sorted_keys[1:] != sorted_keys[:-1]), "duplicate (batch, coordinate)"
        for j in range(jn):
            bits = np.array([j >> 2 & 1, j >> 1 & 1, j & 1], np.int64) if jn == 8 else np.zeros(3, np.int64)
            rows = np.concatenate([pb[:, None], b + bits], 1)
            inside = ok & np.all((rows >= lo) & (rows <= hi), 1)
            key = keys(rows, inside)
            at = np.minimum(np.searchsorted(sorted_keys, key), v - 1)
            hit = inside & (sorted_keys[at] == key)
            table[:, j] = np.where(hit, by_key[at], -1)
            if jn == 8:
                wa = [np.where(bits[a] == 1, f[:, a], d(1) - f[:, a]) for a in range(3)]
                wj = (wa[0] * wa[1]) * wa[2]
            else:
                wj = np.ones(k, x.dtype)
            assert wj.dtype == x.dtype
            w[:, j] = np.where(hit, wj, d(0))
    if normalize:
        s = np.zeros(k, x.dtype)
        for j in range(jn):
            s = np.where(table[:, j] >= 0, s + w[:, j], s)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where((table >= 0) & (s != 0)[:, None], w / s[:, None], d(0))
    assert w.dtype == x.dtype
    return table, w


def corners_brute(coords, positions, batch=None, position_batch=None, mode="linear", normalize=False):
    """the same from a dictionary of the coordinates, point by point with scalars of the positions' dtype"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    x = np.asarray(positions)
    d = x.dtype.type
    jn = MODES[mode]
    cb, pb = _batch(len(c), batch), _batch(len(x), position_batch)
    rows = {(int(cb[i]),) + tuple(int(a) for a in c[i]): i for i in range(len(c))}
    assert len(rows) == len(c)
    table, w = np.full((len(x), jn), -1, np.int32), np.zeros((len(x), jn), x.dtype)
    for i in range(len(x)):
        p = [d(a) for a in x[i]]
        if not all(np.isfinite(a) and -LIMIT <= float(a) < LIMIT for a in p):
            continue
        if jn == 1:
            cell = tuple(int(np.floor(a + d(0.5))) for a in p)
            table[i, 0] = rows.get((int(pb[i]),) + cell, -1)
            w[i, 0] = d(table[i, 0] >= 0)
            continue
        b = [np.floor(a) for a in p]
        f = [a - fl for a, fl in zip(p, b)]
        s = d(0)
        for j in range(8):
            bits = (j >> 2 & 1, j >> 1 & 1, j & 1)
            r = rows.get((int(pb[i]),) + tuple(int(fl) + bit for fl, bit in zip(b, bits)), -1)
            if r < 0:
                continue
            wa = [fa if bit else d(1) - fa for fa, bit in zip(f, bits)]
            table[i, j], w[i, j] = r, d(d(wa[0] * wa[1]) * wa[2])
            s = d(s + w[i, j])
        if normalize:
            w[i] = [d(a / s) if t >= 0 and s != 0 else d(0) for a, t in zip(w[i], table[i])]
    return table, w                                                      # (nearest: normalize divides 1 by 1)


def weights_of(weights, kind):
    """the weights a fold of `kind` multiplies by: fp64 for "f64", fp32 otherwise -- cast once from the table's (one rounding when the
    positions were fp64 and the features are not)"""
    return np.ascontiguousarray(weights).astype(fold_type(kind))


def forward(feat, table, weights, kind):
    """feat [V, C] in the fold type, table / weights [K, J] -> out [K, C] in the fold type, before the final rounding:
    0, then + (w[r, j] * feat[table[r, j]]) per present j in ascending order, a rounding after the product and one after the sum"""
    d = fold_type(kind)
    feat, w = np.asarray(feat), weights_of(weights, kind)
    assert feat.dtype == d
    k, jn = table.shape
    acc = np.zeros((k, feat.shape[1]), d)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(jn):
            e = table[:, j].astype(np.int64)
            here = (e >= 0)[:, None]
            if not here.any():
                continue
            prod = w[:, j, None] * feat[np.maximum(e, 0)]
            acc = np.where(here, acc + prod, acc)
    assert acc.dtype == d
    return acc


def transpose(grad, table, weights, num_voxels, kind):
    """grad [K, C] in the fold type -> [V, C] in the fold type, before the final rounding: voxel v is 0, then + (w_flat[e] * grad[e // J])
    over the entries e of the flattened table that name v, in ascending e.  One pass per rank of an entry inside its voxel"""
    d = fold_type(kind)
    grad, w = np.asarray(grad), weights_of(weights, kind).reshape(-1)
    assert grad.dtype == d
    jn = table.shape[1]
    flat = table.reshape(-1).astype(np.int64)
    acc = np.zeros((num_voxels, grad.shape[1]), d)
    e = np.nonzero(flat >= 0)[0]
    e = e[np.argsort(flat[e], kind="stable")]                            # by voxel, ascending entry inside one
    vox = flat[e]
    first = np.searchsorted(vox, vox, side="left")
    rank = np.arange(len(e)) - first
    with np.errstate(invalid="ignore", over="ignore"):
        for rk in range(int(rank.max()) + 1 if len(e) else 0):
            sel = e[rank == rk]
            prod = w[sel, None] * grad[sel // jn]
            acc[flat[sel]] = acc[flat[sel]] + prod
    assert acc.dtype == d
    return acc


def entries_per_voxel(table, num_voxels):
    return np.bincount(table.reshape(-1)[table.reshape(-1) >= 0], minlength=num_voxels)
