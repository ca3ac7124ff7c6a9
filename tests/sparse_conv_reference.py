"""The numpy model of d3d_amd.voxel.sparse_conv (SparseConvMap / sparse_conv3d / sparse_inverse_conv3d), written from the operator's
contract and from nothing else: the outputs come from a Python dict keyed on (batch, x, y, z) filled by the candidate walk in (v, k)
order, the convolutions and their gradients are fp64 einsums over indexed rows."""
from math import gcd

import numpy as np

import voxel_conv_reference as vref

triple = vref.triple
same_bits = vref.same_bits


def columns(kernel_size):
    """[K, 3] int64: (ix, iy, iz) of column k = (ix * ky + iy) * kz + iz, uncentred"""
    ks = triple(kernel_size)
    assert all(1 <= k <= 7 for k in ks)
    return np.stack(np.meshgrid(*[np.arange(k) for k in ks], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)


def out_shape(spatial_shape, kernel_size, stride, padding=0, dilation=1):
    """dense conv3d's output size per axis"""
    return tuple((n + 2 * p - d * (k - 1) - 1) // s + 1
                 for n, k, s, p, d in zip(triple(spatial_shape), triple(kernel_size), triple(stride), triple(padding), triple(dilation)))


def fanout(kernel_size, stride, dilation=1):
    """P: the most outputs one input can feed, the product over the axes of ceil(k / (s / gcd(s, d)))"""
    p = 1
    for k, s, d in zip(triple(kernel_size), triple(stride), triple(dilation)):
        p *= -(-k // (s // gcd(s, d)))
    return p


def _batch(coords, batch):
    return np.zeros(len(coords), np.int64) if batch is None else np.asarray(batch, np.int64)


def candidates(coords, kernel_size, stride, padding=0, dilation=1, spatial_shape=None):
    """-> (valid [V, K] bool, out [V, K, 3] int64): whether input v has an output through column k, and which (numpy's // and %
    floor, as the contract asks)"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    st, pad, dil = (np.array(triple(x), np.int64) for x in (stride, padding, dilation))
    num = c[:, None, :] + pad - columns(kernel_size)[None] * dil
    valid, out = np.all(num % st == 0, -1), num // st
    if spatial_shape is not None:
        assert np.all(c >= 0) and np.all(c < np.array(triple(spatial_shape))), "an input outside spatial_shape"
        size = np.array(out_shape(spatial_shape, kernel_size, stride, padding, dilation))
        assert np.all(size >= 1)
        valid &= np.all((out >= 0) & (out < size), -1)
    return valid, out


def build(coords, kernel_size, stride, padding=0, dilation=1, batch=None, spatial_shape=None):
    """-> (out_coords [Vout, 3] int64, out_batch [Vout] int64, table_out [Vout, K] int32, table_in [V, K] int32): the walk over the
    candidates (v, k) in ascending v * K + k, a new output row for every (batch, coordinate) not seen before"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    b = _batch(c, batch)
    assert len(set(zip(b.tolist(), *c.T.tolist()))) == len(c), "duplicate (batch, coordinate)"
    valid, out = candidates(c, kernel_size, stride, padding, dilation, spatial_shape)
    kk = valid.shape[1]
    vs, cols = np.nonzero(valid)                                   # row-major: ascending v * K + k
    rows, where = {}, []
    for key in zip(b[vs].tolist(), *out[vs, cols].T.tolist()):
        where.append(rows.setdefault(key, len(rows)))
    where = np.array(where, np.int64)
    table_in = np.full((len(c), kk), -1, np.int32)
    table_out = np.full((len(rows), kk), -1, np.int32)
    table_in[vs, cols] = where
    assert np.all(table_out[where, cols] == -1)
    table_out[where, cols] = vs
    keys = np.array(list(rows), np.int64).reshape(-1, 4)
    return keys[:, 1:].copy(), keys[:, 0].copy(), table_out, table_in


def build_brute(coords, kernel_size, stride, padding=0, dilation=1, batch=None, spatial_shape=None):
    """the same from all pairs (input row, cell of the output box): the pair fills column k when in - (out * stride - padding) is
    (ix, iy, iz) * dilation; the active cells are the ones some input feeds, numbered by their smallest v * K + k.  Small scenes only"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    b = _batch(c, batch)
    ks, st, pad, dil = (np.array(triple(x), np.int64) for x in (kernel_size, stride, padding, dilation))
    kk = int(np.prod(ks))
    lo = -((-(c.min(0) + pad - (ks - 1) * dil)) // st)             # ceil
    hi = (c.max(0) + pad) // st
    if spatial_shape is not None:
        lo, hi = np.maximum(lo, 0), np.minimum(hi, np.array(out_shape(spatial_shape, kernel_size, stride, padding, dilation)) - 1)
    axes = [np.arange(l, h + 1) for l, h in zip(lo, hi)]
    cells = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    ids = np.unique(b)
    cells, cell_b = np.tile(cells, (len(ids), 1)), np.repeat(ids, len(cells))
    diff = c[None, :, :] - (cells[:, None, :] * st - pad)          # [cell, v, 3]
    step = diff // dil
    hit = np.all((diff % dil == 0) & (step >= 0) & (step < ks), -1) & (cell_b[:, None] == b[None, :])
    r, v = np.nonzero(hit)
    col = (step[r, v, 0] * ks[1] + step[r, v, 1]) * ks[2] + step[r, v, 2]
    first = np.full(len(cells), np.iinfo(np.int64).max)
    np.minimum.at(first, r, v * kk + col)
    active = np.nonzero(first < np.iinfo(np.int64).max)[0]
    order = active[np.argsort(first[active], kind="stable")]
    number = np.full(len(cells), -1, np.int64)
    number[order] = np.arange(len(order))
    table_out = np.full((len(order), kk), -1, np.int32)
    table_in = np.full((len(c), kk), -1, np.int32)
    table_out[number[r], col] = v
    table_in[v, col] = number[r]
    return cells[order], cell_b[order], table_out, table_in


def gather(feat, tab):
    """[V, C], [R, K] -> [R, K, C]: feat[tab[r, k]], a zero row for -1 (V may be 0)"""
    padded = np.concatenate([feat, np.zeros((1,) + feat.shape[1:], feat.dtype)])
    return padded[np.where(tab < 0, len(feat), tab).astype(np.int64)]


def conv(feat, tab, weight, bias=None):
    """fp64: out[r] = sum_k feat[tab[r, k]] @ weight[k] (+ bias)"""
    out = np.einsum("rki,kio->ro", gather(feat.astype(np.float64), tab), weight.astype(np.float64))
    return out if bias is None else out + bias.astype(np.float64)


def conv_backward(feat, tab, tab_back, weight, grad_out):
    """fp64 -> (grad_features, grad_weight [K, Cin, Cout], grad_bias [Cout]) of conv(feat, tab, ..); tab_back is the transposed map
    (tab[r, k] == v <=> tab_back[v, k] == r): grad_features[v] = sum_k grad_out[tab_back[v, k]] @ weight[k]^T, unmirrored"""
    f, w, g = feat.astype(np.float64), weight.astype(np.float64), grad_out.astype(np.float64)
    gf = np.einsum("vko,kio->vi", gather(g, tab_back), w)
    gw = np.einsum("rki,ro->kio", gather(f, tab), g)
    return gf, gw, g.sum(0)


def bounds(feat, tab, tab_back, weight, grad_out, eps, bias=None):
    """The dot-product bound of every output, in the form of voxel_conv_reference.bounds: (n + 2) eps sum|a||b| with n the reduction
    length -- K Cin for the forward, K Cout for grad_features, the row count of the output for grad_weight and grad_bias.
    -> (out, grad_features, grad_weight, grad_bias)"""
    f, w, g = np.abs(feat.astype(np.float64)), np.abs(weight.astype(np.float64)), np.abs(grad_out.astype(np.float64))
    k, cin, cout = weight.shape
    rows = len(tab)
    m_out = conv(f, tab, w, None if bias is None else np.abs(bias))
    m_gf, m_gw, m_gb = conv_backward(f, tab, tab_back, w, g)
    return (k * cin + 2) * eps * m_out, (k * cout + 2) * eps * m_gf, (rows + 2) * eps * m_gw, (rows + 2) * eps * m_gb


# ---------------------------------------------------------------- a replay of vstride.hip's output box, key and capacity
def frame(coords, kernel_size, stride, padding=0, dilation=1, batch=None, spatial_shape=None):
    """-> (lo [3], span [3], batch lo, batch span, log2cap): the output box the kernel derives from the input bounds -- the first
    output the smallest input can feed through the last column up to the last one the largest input can feed through the first,
    clipped by spatial_shape -- and the capacity it uses: the smallest power of two >= max(64, 2 min(V P, cells of the box))"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    b = _batch(c, batch)
    ks, st, pad, dil = (triple(x) for x in (kernel_size, stride, padding, dilation))
    lo = [-((-(int(c[:, a].min()) + pad[a] - (ks[a] - 1) * dil[a])) // st[a]) for a in range(3)]
    hi = [(int(c[:, a].max()) + pad[a]) // st[a] for a in range(3)]
    if spatial_shape is not None:
        size = out_shape(spatial_shape, ks, st, pad, dil)
        lo, hi = [max(x, 0) for x in lo], [min(x, n - 1) for x, n in zip(hi, size)]
    span = [max(h - l + 1, 0) for l, h in zip(lo, hi)]
    b_lo, b_span = int(b.min()), int(b.max()) - int(b.min()) + 1
    cells = span[0] * span[1] * span[2] * b_span
    return lo, span, b_lo, b_span, vref.hash_log2cap(min(len(c) * fanout(ks, st, dil), cells))


def out_keys(out_coords, out_batch, fr):
    """the mixed-radix key of every output over the box of `frame`: ((b sx + x) sy + y) sz + z on the positions inside the box"""
    lo, span, b_lo, _, _ = fr
    rel = [(np.asarray(out_batch, np.int64) - b_lo).tolist()] + [(out_coords[:, a] - lo[a]).tolist() for a in range(3)]
    assert all(0 <= min(r) and max(r) < s for r, s in zip(rel[1:], span))
    return [((b * span[0] + x) * span[1] + y) * span[2] + z for b, x, y, z in zip(*rel)]
