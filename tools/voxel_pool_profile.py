"""voxel_pool (vpool.hip) against what a user writes today for the same reduction -- torch's atomic scatter operators -- on the same
device, one process, HIP events:
  sum   voxel_pool(f, idx, 'sum')     vs  zeros(V, C).index_add_(0, m, f)
  mean  voxel_pool(f, idx, 'mean')    vs  zeros(V, C).index_reduce_(0, m, f, 'mean', include_self=False)
  max   voxel_pool(f, idx, 'max')     vs  zeros(V, C).scatter_reduce_(0, m[:, None].expand(-1, C), f, 'amax', include_self=False)
  max f+b  the same two with the gradient of (out * w).sum() through autograd
and the index build (VoxelIndex: once per frame, shared by every layer and every backward) on a line of its own.
Workloads, C = 16 and 64 in fp32:
  lidar 1M     synth.lidar_like(1_000_000) through the sparse VoxelGenerator at config 2's grid (0.1 m voxels, max 32 points, trim)
  lidar 120k   synth.lidar_like(120_000), the same generator
  pillars 120k the same 120 k points in 0.16 m pillars that span the whole z range: the crowded case
torch's operators take no -1: where the mapping holds any, the mapped rows are gathered for them OUTSIDE the timed region.
Per workload the variants alternate inside every round; WARMUP rounds are dropped, then the median [min .. max] over the timed
rounds in ms.  Each voxel_pool line also states the compulsory bytes -- K' C 4 read + V C 4 written (+ V C 4 for `arg` when a
gradient is wanted) + the index (K' 4 + (V + 1) 8) -- and the fraction of the 8 TB/s HBM peak they reach at the median.
Before anything is timed the results are compared: max bit for bit, sum / mean to 1e-4 of the largest |value|.
usage: python tools/voxel_pool_profile.py [out.txt]   (writes profiles/voxel_pool_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                             # noqa: E402
from d3d_amd.voxel import VoxelGenerator, VoxelIndex, voxel_pool                      # noqa: E402

WARMUP, ROUNDS = 3, 20
HBM_PEAK = 8e12
CHANNELS = (16, 64)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def lidar_mapping(n):
    pts = torch.from_numpy(synth.lidar_like(n, 0)).cuda()
    sp = VoxelGenerator(synth.KITTI_BOUNDS, synth.KITTI_SHAPE, max_points=32, max_points_filter="trim")(pts)
    return sp.points_mapping.clone(), int(sp.coords.shape[0])


def pillar_mapping(n, size=0.16):
    """pillar id of every point inside the range, numbered densely (torch.unique): no cap on the points of a pillar"""
    pts = torch.from_numpy(synth.lidar_like(n, 0)).cuda()
    b = synth.KITTI_BOUNDS
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    inside = (x >= b[0]) & (x < b[1]) & (y >= b[2]) & (y < b[3]) & (z >= b[4]) & (z < b[5])
    ny = int(round((b[3] - b[2]) / size))
    cell = ((x[inside] - b[0]) / size).floor().long() * ny + ((y[inside] - b[2]) / size).floor().long()
    uniq, inv = torch.unique(cell, return_inverse=True)
    return inv.contiguous(), int(uniq.numel())


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "voxel_pool_profile.txt")
    assert torch.cuda.is_available(), "voxel_pool_profile needs a GPU"
    torch.cuda.set_device(0)
    lines = ["%s; fp32; %d warm-up rounds, then per variant the median [min .. max] of %d timed rounds in ms, variants alternating "
             "inside a round, HIP events around each; bytes = compulsory traffic of the voxel_pool call, %% = of the 8 TB/s HBM peak"
             % (torch.cuda.get_device_name(0), WARMUP, ROUNDS)]
    print(lines[0], flush=True)
    for name, (m, v) in (("lidar 1M", lidar_mapping(1_000_000)), ("lidar 120k", lidar_mapping(120_000)), ("pillars 120k", pillar_mapping(120_000))):
        k = int(m.numel())
        idx = VoxelIndex(m, v)
        kept = torch.nonzero(m >= 0)[:, 0]
        mk = m[kept]
        cnt = torch.bincount(mk, minlength=v)
        build = [event_ms(lambda: VoxelIndex(m, v)) for _ in range(WARMUP + ROUNDS)][WARMUP:]
        lines.append("%s: K = %d points (%d mapped), V = %d voxels, points per voxel: median %d, max %d" %
                     (name, k, idx.num_mapped, v, int(cnt.float().median()), int(cnt.max())))
        lines.append("  %-14s %-30s   (the read-back included; once per frame, every layer and backward reuses it)" %
                     ("index build", "%.4f [%.4f .. %.4f]" % (float(np.median(build)), min(build), max(build))))
        print("\n".join(lines[-2:]), flush=True)
        for c in CHANNELS:
            f = torch.randn(k, c, device="cuda")
            fk = f[kept].contiguous() if idx.num_mapped != k else f
            w = torch.randn(v, c, device="cuda")
            col = mk[:, None].expand(-1, c)

            def pool(red):
                return lambda: voxel_pool(f, idx, reduction=red)

            def pool_fb():
                x = f.detach().requires_grad_(True)
                (voxel_pool(x, idx, reduction="max") * w).sum().backward()
                return x.grad

            def t_sum():
                return torch.zeros(v, c, device="cuda").index_add_(0, mk, fk)

            def t_mean():
                return torch.zeros(v, c, device="cuda").index_reduce_(0, mk, fk, "mean", include_self=False)

            def t_max(x=None):
                return torch.zeros(v, c, device="cuda").scatter_reduce_(0, col, fk if x is None else x, "amax", include_self=False)

            def t_max_fb():
                x = fk.detach().requires_grad_(True)
                (torch.zeros(v, c, device="cuda").scatter_reduce(0, col, x, "amax", include_self=False) * w).sum().backward()
                return x.grad

            ours = {"sum": pool("sum"), "mean": pool("mean"), "max": pool("max"), "max f+b": pool_fb}
            theirs = {"sum": t_sum, "mean": t_mean, "max": t_max, "max f+b": t_max_fb}
            assert torch.equal(ours["max"](), t_max()), "max differs from scatter_reduce_(amax)"
            for red in ("sum", "mean"):
                a, b = ours[red](), theirs[red]()
                assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()), red
            ms = {(who, red): [] for who in ("pool", "torch") for red in ours}
            for r in range(WARMUP + ROUNDS):
                for red in ours:
                    for who, fn in (("pool", ours[red]), ("torch", theirs[red])):
                        t = event_ms(fn)
                        if r >= WARMUP:
                            ms[who, red].append(t)
            for red in ours:
                p, t = ms["pool", red], ms["torch", red]
                row = idx.num_mapped * c * 4 + v * c * 4 + idx.num_mapped * 4 + (v + 1) * 8
                if red == "max f+b":                     # arg written and read, the gradient [V, C] read, [K, C] written
                    row += 2 * v * c * 4 + v * c * 4 + k * c * 4 + k * 8
                cell = lambda x: "%.4f [%.4f .. %.4f]" % (float(np.median(x)), min(x), max(x))      # noqa: E731
                lines.append("  C=%-3d %-8s pool %-28s torch %-28s torch/pool %6.2fx   %6.1f MB, %4.1f %% of HBM peak" %
                             (c, red, cell(p), cell(t), np.median(t) / np.median(p), row / 1e6, 100 * row / (np.median(p) * 1e-3) / HBM_PEAK))
                print(lines[-1], flush=True)
            del f, fk, w, col
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
