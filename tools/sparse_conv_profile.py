"""SparseConvMap / sparse_conv3d / sparse_inverse_conv3d (vstride.hip) against what a user writes today with torch alone, on the voxels
of a 1 M-point LiDAR-like frame at the 704 x 800 x 40 grid:

  map       SparseConvMap(coords, 3, 2, 1, spatial_shape)  vs  linear keys of every candidate's output over the output grid,
                                                               torch.unique (sorted), a searchsorted per column for table_in and a
                                                               scatter for table_out; both with their read-back of Vout
  conv      sparse_conv3d forward, forward+backward        vs  the same convolution from the torch tables: per column a row gather,
                                                               a GEMM and an index_add_ (float atomics), autograd for the backward;
                                                               the per-column row lists are built once per frame, outside the
                                                               timing, as the map is
  inverse   sparse_inverse_conv3d forward of a k2 s2 p0 map vs  the same from the torch tables of that map

The torch map numbers its outputs by ascending key, ours by first candidate: the results are compared through the coordinate match
(the permutation between the two row orders), the tables exactly, the convolutions within 1e-3 of each other.

Timing: WARMUP untimed rounds, then ROUNDS rounds in which the variants alternate; HIP events around each call; median [min .. max]
in ms.

usage: python tools/sparse_conv_profile.py [out.txt]   (writes profiles/sparse_conv_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                                          # noqa: E402
from d3d_amd.voxel import SparseConvMap, VoxelGenerator, sparse_conv3d, sparse_inverse_conv3d      # noqa: E402

WARMUP, ROUNDS = 3, 20
CHANNELS = (16, 64)
SHAPE = synth.KITTI_SHAPE


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def out_size(k, s, p):
    return tuple((n + 2 * p - (k - 1) - 1) // s + 1 for n in SHAPE)


def torch_map(coords, k, s, p):
    """-> (sorted output keys [Vout], table_in [V, K] int64, table_out [Vout, K] int64), rows in ascending key order, -1 = none"""
    ox, oy, oz = out_size(k, s, p)
    keys, valid = [], []
    for ix in range(k):
        for iy in range(k):
            for iz in range(k):
                num = coords + p - torch.tensor([ix, iy, iz], device=coords.device)
                o = torch.div(num, s, rounding_mode="floor")
                ok = ((num - o * s) == 0).all(1) & (o >= 0).all(1) & (o[:, 0] < ox) & (o[:, 1] < oy) & (o[:, 2] < oz)
                keys.append((o[:, 0] * oy + o[:, 1]) * oz + o[:, 2])
                valid.append(ok)
    keys, valid = torch.stack(keys, 1), torch.stack(valid, 1)
    uniq = torch.unique(keys[valid])                                # (sorted; its length is the read-back)
    table_in = torch.where(valid, torch.searchsorted(uniq, keys.reshape(-1)).reshape(keys.shape), -1)
    table_out = torch.full((len(uniq), keys.shape[1]), -1, dtype=torch.int64, device=coords.device)
    v, col = torch.nonzero(valid, as_tuple=True)
    table_out[table_in[v, col], col] = v
    return uniq, table_in, table_out


def torch_columns(table):
    """per column the rows that read through it and the rows they read: built once per frame, like the map"""
    cols = []
    for k in range(table.shape[1]):
        rows = torch.nonzero(table[:, k] >= 0)[:, 0]
        cols.append((rows, table[rows, k].contiguous()))
    return cols


def torch_conv(x, cols, w, rows):
    """out[r] = sum_k x[table[r, k]] @ w[k]: per column a row gather, a GEMM, an index_add_"""
    out = torch.zeros((rows, w.shape[2]), dtype=x.dtype, device=x.device)
    for k, (dst, src) in enumerate(cols):
        out.index_add_(0, dst, x[src] @ w[k])
    return out


def cell(x):
    return "%.3f [%.3f .. %.3f]" % (float(np.median(x)), min(x), max(x))


def match(cmap, uniq, k, s, p):
    """the torch row of every row of ours, through the coordinates"""
    _, oy, oz = out_size(k, s, p)
    o = cmap.out_coords
    perm = torch.searchsorted(uniq, (o[:, 0] * oy + o[:, 1]) * oz + o[:, 2])
    assert len(uniq) == cmap.num_out and torch.equal(uniq[perm], (o[:, 0] * oy + o[:, 1]) * oz + o[:, 2]), "the output sets differ"
    return perm


def close(a, b):
    return float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())


def race(legs, lines, label):
    ms = {(who, leg): [] for who in (0, 1) for leg in legs}
    for r in range(WARMUP + ROUNDS):
        for leg in legs:
            for who in (0, 1):
                t = event_ms(legs[leg][who])
                if r >= WARMUP:
                    ms[who, leg].append(t)
    for leg in legs:
        lines.append("  %-22s ours %-29s torch %-30s torch/ours %6.2fx" % (label + " " + leg, cell(ms[0, leg]), cell(ms[1, leg]),
                                                                          np.median(ms[1, leg]) / np.median(ms[0, leg])))
        print(lines[-1], flush=True)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_conv_profile.txt")
    assert torch.cuda.is_available(), "sparse_conv_profile needs a GPU"
    torch.cuda.set_device(0)
    pts = torch.from_numpy(synth.lidar_like(1_000_000, 0)).cuda()
    coords = VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, max_points=32, max_points_filter="trim")(pts).coords.long().contiguous()
    v = coords.shape[0]
    cmap = SparseConvMap(coords, 3, 2, 1, spatial_shape=SHAPE)
    uniq, t_in, t_out = torch_map(coords, 3, 2, 1)
    perm = match(cmap, uniq, 3, 2, 1)
    assert torch.equal(torch.where(cmap.table_in >= 0, perm[cmap.table_in.long().clamp(min=0)], -1), t_in), "table_in differs"
    assert torch.equal(cmap.table_out.long(), t_out[perm]), "table_out differs"
    lines = ["%s; fp32; %d warm-up rounds, then per variant the median [min .. max] of %d timed rounds in ms, variants alternating "
             "inside a round, HIP events around each" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS),
             "lidar 1M: V = %d voxels; k3 s2 p1 on %r: Vout = %d, K = 27, %d entries (%.2f per input, %.2f per output)" %
             (v, tuple(SHAPE), cmap.num_out, cmap.num_entries, cmap.num_entries / v, cmap.num_entries / cmap.num_out)]
    print("\n".join(lines), flush=True)
    race({"build": (lambda: SparseConvMap(coords, 3, 2, 1, spatial_shape=SHAPE), lambda: torch_map(coords, 3, 2, 1))}, lines, "map k3 s2 p1")
    lines[-1] += "   (the read-backs included; once per frame and layer)"
    cols = torch_columns(t_out)
    for c in CHANNELS:
        x = torch.randn(v, c, device="cuda")
        w = torch.randn(27, c, c, device="cuda") / (27 * c) ** 0.5
        g = torch.randn(cmap.num_out, c, device="cuda")

        def ours_fb():
            a, b = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
            sparse_conv3d(a, cmap, b).backward(g)
            return a.grad, b.grad

        def torch_fb():
            a, b = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
            torch_conv(a, cols, b, len(uniq)).backward(g[perm_inv])
            return a.grad, b.grad

        perm_inv = torch.empty_like(perm)
        perm_inv[perm] = torch.arange(len(perm), device="cuda")
        assert close(sparse_conv3d(x, cmap, w), torch_conv(x, cols, w, len(uniq))[perm]), "the convolutions differ"
        (a, b), (ta, tb) = ours_fb(), torch_fb()
        assert close(a, ta) and close(b, tb), "the gradients differ"
        race({"fwd": (lambda: sparse_conv3d(x, cmap, w), lambda: torch_conv(x, cols, w, len(uniq))), "f+b": (ours_fb, torch_fb)}, lines,
             "conv C=%d" % c)
        del x, w, g
    # one inverse convolution: k2 s2 p0, back from the halved grid to the input sites
    cmap2 = SparseConvMap(coords, 2, 2, 0, spatial_shape=SHAPE)
    uniq2, t_in2, _ = torch_map(coords, 2, 2, 0)
    perm2 = match(cmap2, uniq2, 2, 2, 0)
    cols2 = torch_columns(t_in2)
    lines.append("k2 s2 p0: Vout = %d, K = 8, %d entries" % (cmap2.num_out, cmap2.num_entries))
    for c in CHANNELS:
        z = torch.randn(cmap2.num_out, c, device="cuda")
        w = torch.randn(8, c, c, device="cuda") / (8 * c) ** 0.5
        zt = torch.empty_like(z)
        zt[perm2] = z                                               # the same rows in the torch map's order
        assert close(sparse_inverse_conv3d(z, cmap2, w), torch_conv(zt, cols2, w, v)), "the inverse convolutions differ"
        race({"fwd": (lambda: sparse_inverse_conv3d(z, cmap2, w), lambda: torch_conv(zt, cols2, w, v))}, lines, "inverse C=%d" % c)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
