"""The fused table convolution (csrc/vconv.hip, method="fused") against the gather route and against what a user writes with torch
alone, on the voxels of a 1 M-point LiDAR-like frame at the 704 x 800 x 40 grid -- the frame and the protocol of voxel_conv_profile.py
and sparse_conv_profile.py:

  subm      subm_conv3d, K = 27                         inverse   sparse_inverse_conv3d of a k2 s2 p0 map, K = 8
  strided   sparse_conv3d of a k3 s2 p1 map, K = 27

  fp32        fused  vs  gather (method=None)  vs  torch: per column a row gather, a GEMM and an index_add_ (float atomics), autograd
              for the backward; the per-column row lists are built once per frame, outside the timing, as the tables are
  bf16, fp16  fused  vs  the same torch convolution run in that dtype

Timing: WARMUP untimed rounds, then ROUNDS rounds in which the variants alternate; HIP events around each call; median [min .. max]
in ms.  The results are compared before anything is timed.  peak: the most memory a forward call holds beyond what was allocated
before it (MiB) -- the gather route's K-fold buffer shows there, the fused route has none.

usage: python tools/table_conv_profile.py [out.txt]   (writes profiles/table_conv_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                                                        # noqa: E402
from d3d_amd.voxel import SparseConvMap, VoxelGenerator, VoxelNeighbors, sparse_conv3d, sparse_inverse_conv3d, subm_conv3d   # noqa: E402

WARMUP, ROUNDS = 3, 20
CHANNELS = (16, 64)
SHAPE = synth.KITTI_SHAPE
DTYPES = (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_columns(table):
    cols = []
    for k in range(table.shape[1]):
        rows = torch.nonzero(table[:, k] >= 0)[:, 0]
        cols.append((rows, table[rows, k].long().contiguous()))
    return cols


def torch_conv(x, cols, w, rows):
    out = torch.zeros((rows, w.shape[2]), dtype=x.dtype, device=x.device)
    for k, (dst, src) in enumerate(cols):
        out.index_add_(0, dst, x[src] @ w[k])
    return out


def cell(x):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(x)), min(x), max(x))


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def close(a, b, tol):
    return float((a.float() - b.float()).abs().max()) <= tol * float(b.float().abs().max())


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "table_conv_profile.txt")
    assert torch.cuda.is_available(), "table_conv_profile needs a GPU"
    torch.cuda.set_device(0)
    pts = torch.from_numpy(synth.lidar_like(1_000_000, 0)).cuda()
    coords = VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, max_points=32, max_points_filter="trim")(pts).coords.long().contiguous()
    v = coords.shape[0]
    nbrs = VoxelNeighbors(coords)
    down = SparseConvMap(coords, 3, 2, 1, spatial_shape=SHAPE)
    up = SparseConvMap(coords, 2, 2, 0, spatial_shape=SHAPE)
    # name -> (operator, its table owner, the forward table, source rows, output rows)
    ops = {"subm k3": (subm_conv3d, nbrs, nbrs.table, v, v),
           "strided k3 s2 p1": (sparse_conv3d, down, down.table_out, v, down.num_out),
           "inverse k2 s2 p0": (sparse_inverse_conv3d, up, up.table_in, up.num_out, v)}
    lines = ["%s; %d warm-up rounds, then per variant the median [min .. max] of %d timed rounds in ms, variants alternating inside a "
             "round, HIP events around each" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS),
             "lidar 1M: V = %d voxels; subm K = 27, %d entries; k3 s2 p1: Vout = %d, %d entries; k2 s2 p0: Vout = %d, %d entries" %
             (v, nbrs.num_entries, down.num_out, down.num_entries, up.num_out, up.num_entries)]
    print("\n".join(lines), flush=True)
    for name, (op, owner, table, src_rows, rows) in ops.items():
        cols = torch_columns(table)
        k = table.shape[1]
        for c in CHANNELS:
            x32 = torch.randn(src_rows, c, device="cuda")
            w32 = torch.randn(k, c, c, device="cuda") / (k * c) ** 0.5
            g32 = torch.randn(rows, c, device="cuda")
            for label, dt in DTYPES:
                x, w, g = x32.to(dt), w32.to(dt), g32.to(dt)

                def fb(fn):
                    def run():
                        a, b = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
                        fn(a, b).backward(g)
                        return a.grad, b.grad
                    return run

                routes = {"fused": lambda a, b: op(a, owner, b, method="fused"), "torch": lambda a, b: torch_conv(a, cols, b, rows)}
                if dt == torch.float32:
                    routes["gather"] = lambda a, b: op(a, owner, b)
                tol = 1e-3 if dt == torch.float32 else 0.1
                want = torch_conv(x32, cols, w32, rows)
                for r, fn in routes.items():
                    assert close(fn(x, w), want, tol), (name, c, label, r, "forward")
                gx, gw = fb(routes["torch"])()
                for r, fn in routes.items():
                    a, b = fb(fn)()
                    assert close(a, gx, tol) and close(b, gw, tol), (name, c, label, r, "gradients")
                del want, gx, gw, a, b
                legs = {"fwd": {r: (lambda fn=fn: fn(x, w)) for r, fn in routes.items()}, "f+b": {r: fb(fn) for r, fn in routes.items()}}
                ms = {(leg, r): [] for leg in legs for r in routes}
                for n in range(WARMUP + ROUNDS):
                    for leg in legs:
                        for r in routes:
                            t = event_ms(legs[leg][r])
                            if n >= WARMUP:
                                ms[leg, r].append(t)
                peaks = {r: peak_mib(legs["fwd"][r]) for r in routes}
                for leg in legs:
                    med = {r: float(np.median(ms[leg, r])) for r in routes}
                    text = "  %-17s C=%-3d %s %-4s" % (name, c, label, leg) + "".join(" %s %s" % (r, cell(ms[leg, r])) for r in routes)
                    text += "  torch/fused %5.2fx" % (med["torch"] / med["fused"])
                    if "gather" in routes:
                        text += "  gather/fused %5.2fx" % (med["gather"] / med["fused"])
                    if leg == "fwd":
                        text += "  peak MiB" + "".join(" %s %.0f" % (r, peaks[r]) for r in routes)
                    lines.append(text)
                    print(text, flush=True)
            del x32, w32, g32
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
