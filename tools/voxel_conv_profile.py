"""VoxelNeighbors / subm_conv3d (vnbr.hip) against what a user writes today with torch alone, on the voxels of a 1 M-point LiDAR-like
frame at the 704 x 800 x 40 grid (K = 27, dilation 1):

  table     VoxelNeighbors(coords)                   vs  linear keys, one sort, 27 x searchsorted over the sorted keys
  conv f+b  subm_conv3d(x, nbrs, w) forward+backward  vs  the same convolution from that torch table: per column a row gather, a
                                                          GEMM and an index_add_ (float atomics), autograd for the backward;
                                                          the per-column row lists are built once per frame, outside the timing,
                                                          as the table is

Timing: WARMUP untimed rounds, then ROUNDS rounds in which the variants alternate; HIP events around each call; median [min .. max]
in ms.  The torch table is checked against ours before anything is timed, the torch convolution within 1e-3 of ours.

usage: python tools/voxel_conv_profile.py [out.txt]   (writes profiles/voxel_conv_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                             # noqa: E402
from d3d_amd.voxel import VoxelGenerator, VoxelNeighbors, subm_conv3d                 # noqa: E402

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


def torch_table(coords):
    """[V, 27] int64, -1 = none: linear keys over the grid, one sort, a searchsorted per column (the grid's shape is known here;
    VoxelNeighbors measures it)"""
    sx, sy, sz = SHAPE
    keys = (coords[:, 0] * sy + coords[:, 1]) * sz + coords[:, 2]
    skeys, order = torch.sort(keys)
    cols = []
    for ix in (-1, 0, 1):
        for iy in (-1, 0, 1):
            for iz in (-1, 0, 1):
                x, y, z = coords[:, 0] + ix, coords[:, 1] + iy, coords[:, 2] + iz
                inside = (x >= 0) & (x < sx) & (y >= 0) & (y < sy) & (z >= 0) & (z < sz)
                want = (x * sy + y) * sz + z
                pos = torch.searchsorted(skeys, want).clamp_(max=len(skeys) - 1)
                cols.append(torch.where(inside & (skeys[pos] == want), order[pos], -1))
    return torch.stack(cols, 1)


def torch_columns(table):
    """per column the rows that have the neighbour and the neighbours' rows: built once per frame, like the table"""
    cols = []
    for k in range(table.shape[1]):
        rows = torch.nonzero(table[:, k] >= 0)[:, 0]
        cols.append((rows, table[rows, k].contiguous()))
    return cols


def torch_conv(x, cols, w):
    """out[v] = sum_k x[table[v, k]] @ w[k]: per column a row gather, a GEMM, an index_add_"""
    out = torch.zeros((x.shape[0], w.shape[2]), dtype=x.dtype, device=x.device)
    for k, (rows, src) in enumerate(cols):
        out.index_add_(0, rows, x[src] @ w[k])
    return out


def cell(x):
    return "%.3f [%.3f .. %.3f]" % (float(np.median(x)), min(x), max(x))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "voxel_conv_profile.txt")
    assert torch.cuda.is_available(), "voxel_conv_profile needs a GPU"
    torch.cuda.set_device(0)
    pts = torch.from_numpy(synth.lidar_like(1_000_000, 0)).cuda()
    coords = VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, max_points=32, max_points_filter="trim")(pts).coords.long().contiguous()
    v = coords.shape[0]
    nbrs = VoxelNeighbors(coords)
    table = torch_table(coords)
    assert torch.equal(table, nbrs.table.long()), "the torch table differs"
    cols = torch_columns(table)
    lines = ["%s; fp32; %d warm-up rounds, then per variant the median [min .. max] of %d timed rounds in ms, variants alternating "
             "inside a round, HIP events around each" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS),
             "lidar 1M: V = %d voxels, K = 27, %d entries (%.2f neighbours per voxel, itself included)" % (v, nbrs.num_entries, nbrs.num_entries / v)]
    ms = {"ours": [], "torch": []}
    for r in range(WARMUP + ROUNDS):
        for who, fn in (("ours", lambda: VoxelNeighbors(coords)), ("torch", lambda: torch_table(coords))):
            t = event_ms(fn)
            if r >= WARMUP:
                ms[who].append(t)
    lines.append("  table        VoxelNeighbors %-26s torch %-30s torch/ours %6.2fx   (the read-back included; once per frame)" %
                 (cell(ms["ours"]), cell(ms["torch"]), np.median(ms["torch"]) / np.median(ms["ours"])))
    print("\n".join(lines), flush=True)
    for c in CHANNELS:
        x = torch.randn(v, c, device="cuda")
        w = torch.randn(27, c, c, device="cuda") / (27 * c) ** 0.5
        g = torch.randn(v, c, device="cuda")

        def ours_fb():
            a, b = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
            subm_conv3d(a, nbrs, b).backward(g)
            return a.grad, b.grad

        def torch_fb():
            a, b = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
            torch_conv(a, cols, b).backward(g)
            return a.grad, b.grad

        legs = {"fwd": (lambda: subm_conv3d(x, nbrs, w), lambda: torch_conv(x, cols, w)), "f+b": (ours_fb, torch_fb)}
        ref = torch_conv(x, cols, w)
        assert float((subm_conv3d(x, nbrs, w) - ref).abs().max()) <= 1e-3 * float(ref.abs().max()), "the convolutions differ"
        for (a, b), (ta, tb) in ((ours_fb(), torch_fb()),):
            assert float((a - ta).abs().max()) <= 1e-3 * float(ta.abs().max()) and float((b - tb).abs().max()) <= 1e-3 * float(tb.abs().max())
        ms = {(who, leg): [] for who in (0, 1) for leg in legs}
        for r in range(WARMUP + ROUNDS):
            for leg in legs:
                for who in (0, 1):
                    t = event_ms(legs[leg][who])
                    if r >= WARMUP:
                        ms[who, leg].append(t)
        for leg in legs:
            lines.append("  C=%-3d %-5s subm_conv3d %-29s torch %-30s torch/ours %6.2fx" %
                         (c, leg, cell(ms[0, leg]), cell(ms[1, leg]), np.median(ms[1, leg]) / np.median(ms[0, leg])))
            print(lines[-1], flush=True)
        del x, w, g, ref
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
