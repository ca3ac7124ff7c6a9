"""The numpy model of d3d_amd.voxel.conv (VoxelNeighbors / neighbor_gather / subm_conv3d), written from the operator's contract and
from nothing else: the table comes from a Python dict keyed on (batch, x, y, z), the gather is indexing, the convolution an fp64
einsum, the gather's backward the left fold over the columns."""
from itertools import repeat

import numpy as np


def triple(x):
    return tuple(int(a) for a in x) if isinstance(x, (tuple, list)) else (int(x),) * 3


def offsets(kernel_size, dilation=1):
    """[K, 3] int64: the offset of column k = (ix * ky + iy) * kz + iz, ((ix, iy, iz) - (k* - 1) / 2) * dilation"""
    ks, dil = triple(kernel_size), triple(dilation)
    assert all(k % 2 == 1 and 1 <= k <= 7 for k in ks) and all(d >= 1 for d in dil)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in ks], indexing="ij"), -1).reshape(-1, 3)
    return (idx - (np.array(ks) - 1) // 2) * np.array(dil)


def _batch(coords, batch):
    return np.zeros(len(coords), np.int64) if batch is None else np.asarray(batch, np.int64)


def table(coords, kernel_size=3, dilation=1, batch=None):
    """-> [V, K] int32: the row at every offset, -1 where no row has that coordinate and the same batch value"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    b = _batch(c, batch).tolist()
    rows = {}
    for i, key in enumerate(zip(b, *c.T.tolist())):
        assert key not in rows, "duplicate (batch, coordinate)"
        rows[key] = i
    off = offsets(kernel_size, dilation)
    out = np.empty((len(c), len(off)), np.int32)
    for k, o in enumerate(off):
        out[:, k] = list(map(rows.get, zip(b, *(c + o).T.tolist()), repeat(-1)))
    return out


def table_brute(coords, kernel_size=3, dilation=1, batch=None):
    """the same table from all V^2 pairs of rows: the pair (v, u) fills column k of row v when coords[u] - coords[v] is offset k"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    b = _batch(c, batch)
    ks, dil = np.array(triple(kernel_size)), np.array(triple(dilation))
    diff = c[None, :, :] - c[:, None, :]                          # [v, u, 3]
    step = diff // dil + (ks - 1) // 2                            # the column index per axis, where there is one
    hit = np.all((diff % dil == 0) & (step >= 0) & (step < ks), -1) & (b[:, None] == b[None, :])
    v, u = np.nonzero(hit)
    out = np.full((len(c), int(np.prod(ks))), -1, np.int32)
    s = step[v, u]
    out[v, (s[:, 0] * ks[1] + s[:, 1]) * ks[2] + s[:, 2]] = u
    return out


def gather(feat, tab, mirrored=False):
    """[V, C], [R, K] -> [R, K, C]: feat[tab[r, kk]], kk = K-1-k when mirrored; a zero row for -1"""
    t = tab[:, ::-1] if mirrored else tab
    out = feat[np.maximum(t, 0).astype(np.int64)]
    out[t < 0] = 0
    return out


def gather_backward(grad, tab):
    """[V, K, C] -> [V, C]: grad_feat[u] = grad[tab[u, K-1], 0] + grad[tab[u, K-2], 1] + ... folded in that order in the dtype
    (an absent neighbour adds +0)"""
    v, k, c = grad.shape
    cols = np.arange(k)
    src = tab[:, ::-1].astype(np.int64)
    g = grad[np.maximum(src, 0), cols[None, :]]                   # [V, K, C]: row [tab[u, K-1-k], k]
    g[src < 0] = 0
    acc = g[:, 0].copy()
    for j in range(1, k):
        acc = acc + g[:, j]
    return acc


def conv(feat, tab, weight, bias=None):
    """fp64: out[v] = sum_k feat[tab[v, k]] @ weight[k] (+ bias)"""
    out = np.einsum("vki,kio->vo", gather(feat.astype(np.float64), tab), weight.astype(np.float64))
    return out if bias is None else out + bias.astype(np.float64)


def conv_backward(feat, tab, weight, grad_out):
    """fp64 -> (grad_features [V, Cin], grad_weight [K, Cin, Cout], grad_bias [Cout])"""
    f, w, g = feat.astype(np.float64), weight.astype(np.float64), grad_out.astype(np.float64)
    gf = np.einsum("vko,kio->vi", gather(g, tab, mirrored=True), w)
    gw = np.einsum("vki,vo->kio", gather(f, tab), g)
    return gf, gw, g.sum(0)


def conv_magnitudes(feat, tab, weight, grad_out, bias=None):
    """the sums of absolute products behind every output of conv and conv_backward: what the rounding bounds scale with
    -> (out, grad_features, grad_weight, grad_bias)"""
    f, w, g = np.abs(feat.astype(np.float64)), np.abs(weight.astype(np.float64)), np.abs(grad_out.astype(np.float64))
    return (conv(f, tab, w, None if bias is None else np.abs(bias)),) + conv_backward(f, tab, w, g)


def bounds(feat, tab, weight, grad_out, eps, bias=None):
    """The dot-product bound of every output.  A sum of n products computed in any order in a format of unit roundoff u = eps / 2
    is within n u sum|a||b| of the exact value (first order; the + 2 covers the higher orders and the bias addition), and two
    such computations within n eps sum|a||b| of each other.  n = K Cin for the forward, K Cout for grad_features, V for
    grad_weight and grad_bias."""
    v, cin = feat.shape
    k, _, cout = weight.shape
    m_out, m_gf, m_gw, m_gb = conv_magnitudes(feat, tab, weight, grad_out, bias)
    return (k * cin + 2) * eps * m_out, (k * cout + 2) * eps * m_gf, (v + 2) * eps * m_gw, (v + 2) * eps * m_gb


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    word = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(word), b.view(word))


# ---------------------------------------------------------------- a replay of vnbr.hip's hash table (key, hash, linear probing)
HASH_MIX = 0x9e3779b97f4a7c15


def hash_log2cap(v):
    """the table's capacity: the smallest power of two >= max(2 v, 64)"""
    n = 6
    while (1 << n) < 2 * v:
        n += 1
    return n


def hash_keys(coords, batch=None):
    """the mixed-radix key of every row over the measured spans, ((b sx + x) sy + y) sz + z on the positions inside the box"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    rel = [(_batch(c, batch) - _batch(c, batch).min()).tolist() if batch is not None else [0] * len(c)]
    rel += [(c[:, a] - c[:, a].min()).tolist() for a in range(3)]
    span = [max(r) + 1 for r in rel]
    return [((b * span[1] + x) * span[2] + y) * span[3] + z for b, x, y, z in zip(*rel)]


def hash_home(key, log2cap):
    """the slot a key's probe starts at: the top bits of key * HASH_MIX mod 2^64"""
    return ((key * HASH_MIX) & (2 ** 64 - 1)) >> (64 - log2cap)


def hash_replay(keys, log2cap):
    """the keys inserted in the given order -> (slots: slot -> key, wrapped: the inserts that stepped from the last slot to slot 0).
    The SET of occupied slots does not depend on the order; which key sits where does"""
    cap, slots, wrapped = 1 << log2cap, {}, 0
    for key in keys:
        h, crossed = hash_home(key, log2cap), False
        while h in slots:
            assert slots[h] != key, "duplicate key"
            crossed |= h == cap - 1
            h = (h + 1) % cap
        slots[h] = key
        wrapped += crossed
    return slots, wrapped


def hash_walk(key, slots, log2cap):
    """a look-up of `key` -> (found, probes, crossed the end of the table)"""
    cap, h, probes, crossed = 1 << log2cap, hash_home(key, log2cap), 1, False
    while h in slots and slots[h] != key:
        crossed |= h == cap - 1
        h = (h + 1) % cap
        probes += 1
    return h in slots, probes, crossed
