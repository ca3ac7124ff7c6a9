"""sparse_pool3d (csrc/vtpool.hip) against the two routes a user had without it, on the voxels of a 1 M-point LiDAR-like frame at the
704 x 800 x 40 grid -- the frame and the protocol of table_conv_profile.py:

  strided   a k3 s2 p1 SparseConvMap, K = 27            subm      a VoxelNeighbors of kernel 3, K = 27 (stride-1 "same" pooling)

  pool      sparse_pool3d: one launch forward, one backward
  gather    the gathered [rows, K, C] buffer (d3d_neighbor_gather), absent neighbours masked to -inf for the max, then amax / sum over
            K.  The gather has no half type: the bf16 lines time it on the fp32 inputs.  Its gradient exists through neighbor_gather,
            i.e. for the submanifold table only
  torch     per column a row gather and a scatter_reduce_("amax") / index_add_ (float atomics) into the output, autograd for the
            backward; the per-column row lists are built once per frame, outside the timing, as the tables are

Timing: WARMUP untimed rounds, then ROUNDS rounds in which the variants alternate; HIP events around each call; median [min .. max]
in ms.  The results are compared before anything is timed.  peak: the most memory a forward call holds beyond what was allocated
before it (MiB) -- the gather route's K-fold buffer shows there.  kernel: the launch's own time (d3d_profile_report, HIP events around
the launch, a run of its own) and the bytes of the model of DESIGN.md 4d-4 over it, as a fraction of the 8 TB/s HBM peak -- the
feature rows are counted once per present entry although most of those reads are served by the caches.

usage: python tools/sparse_pool_profile.py [out.txt]   (writes profiles/sparse_pool_profile.txt by default)"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import _lib, synth                                                                  # noqa: E402
from d3d_amd.voxel import SparseConvMap, VoxelGenerator, VoxelNeighbors, neighbor_gather, sparse_pool3d     # noqa: E402
from d3d_amd.voxel.conv import _gather                                                           # noqa: E402

WARMUP, ROUNDS = 3, 20
CHANNELS = (16, 64)
SHAPE = synth.KITTI_SHAPE
DTYPES = (("fp32", torch.float32), ("bf16", torch.bfloat16))
REDUCTIONS = ("max", "sum")
HBM_PEAK = 8e12


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


def torch_pool(x, cols, rows, red):
    if red == "sum":
        out = torch.zeros((rows, x.shape[1]), dtype=x.dtype, device=x.device)
        for dst, src in cols:
            out = out.index_add(0, dst, x[src])
        return out
    out = torch.full((rows, x.shape[1]), float("-inf"), dtype=x.dtype, device=x.device)
    for dst, src in cols:
        out = out.scatter_reduce(0, dst[:, None].expand(-1, x.shape[1]), x[src], "amax", include_self=True)
    return out


def gather_pool(x, owner, view, red):
    """the parent commit's route: [rows, K, C], then the reduction over K (through autograd only where neighbor_gather exists)"""
    g = neighbor_gather(x, owner) if isinstance(owner, VoxelNeighbors) else _gather(x.detach(), view, False)
    if red == "sum":
        return g.sum(1)
    return torch.where((view.table >= 0)[:, :, None], g, g.new_full((), float("-inf"))).amax(1)


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


def kernels(fn, calls=5):
    """-> {launch name: ms per launch} over `calls` calls of fn"""
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.d3d_profile_enable(1)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    lib.d3d_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.d3d_profile_report(buf, len(buf))
    recs = [ln.rsplit(",", 2) for ln in buf.value.decode().strip().splitlines()]
    return {name: float(ms) / int(n) for name, n, ms in recs}


def model_bytes(rows, k, entries, c, elt, arg):
    """the table row, one feature (gradient) row per present entry -- with its int16 winners on the way back of a
    max -- and the output row, with its int16 winners on the way forward"""
    fwd = rows * 4 * k + entries * c * elt + rows * c * (elt + (2 if arg else 0))
    return fwd


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sparse_pool_profile.txt")
    assert torch.cuda.is_available(), "sparse_pool_profile needs a GPU"
    torch.cuda.set_device(0)
    pts = torch.from_numpy(synth.lidar_like(1_000_000, 0)).cuda()
    coords = VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, max_points=32, max_points_filter="trim")(pts).coords.long().contiguous()
    v = coords.shape[0]
    nbrs = VoxelNeighbors(coords)
    down = SparseConvMap(coords, 3, 2, 1, spatial_shape=SHAPE)
    # name -> (owner, its forward view, output rows, entries)
    ops = {"strided k3 s2 p1": (down, down._down, down.num_out, down.num_entries), "subm k3": (nbrs, nbrs._view, v, nbrs.num_entries)}
    lines = ["%s; %d warm-up rounds, then per variant the median [min .. max] of %d timed rounds in ms, variants alternating inside a "
             "round, HIP events around each" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS),
             "lidar 1M: V = %d voxels; subm K = 27, %d entries; k3 s2 p1: Vout = %d, %d entries" %
             (v, nbrs.num_entries, down.num_out, down.num_entries)]
    print("\n".join(lines), flush=True)
    for name, (owner, view, rows, entries) in ops.items():
        cols = torch_columns(view.table)
        k = view.kernel_volume
        has_gather_grad = isinstance(owner, VoxelNeighbors)
        for c in CHANNELS:
            x32 = torch.randn(v, c, device="cuda")
            g32 = torch.randn(rows, c, device="cuda")
            for label, dt in DTYPES:
                x, g = x32.to(dt), g32.to(dt)
                for red in REDUCTIONS:
                    # (the gather route takes fp32 / fp64 only: in the bf16 lines it runs on the fp32 inputs)
                    routes = {"pool": (lambda a: sparse_pool3d(a, owner, red), x, g),
                              "torch": (lambda a: torch_pool(a, cols, rows, red), x, g),
                              "gather": (lambda a: gather_pool(a, owner, view, red), x32, g32)}

                    def fb(r):
                        fn, xin, gin = routes[r]

                        def run():
                            a = xin.detach().requires_grad_(True)
                            fn(a).backward(gin)
                            return a.grad
                        return run

                    want = torch_pool(x, cols, rows, red)
                    got = sparse_pool3d(x, owner, red)
                    if red == "max":
                        assert torch.equal(got, want) and torch.equal(gather_pool(x32, owner, view, red).to(dt), want), (name, c, label, red)
                    else:
                        tol = 1e-4 if dt == torch.float32 else 0.05
                        assert float((got.float() - want.float()).abs().max()) <= tol * float(want.float().abs().max()), (name, c, label, red)
                    if red == "sum":             # (a max's gradient may pick another winner among equal values: bf16 has ties)
                        a, b = fb("pool")(), fb("torch")()
                        tol = 1e-4 if dt == torch.float32 else 0.05
                        assert float((a.float() - b.float()).abs().max()) <= tol * float(b.float().abs().max()), (name, c, label, red, "gradient")
                        del a, b
                    del want, got
                    legs = {"fwd": {r: (lambda r=r: routes[r][0](routes[r][1])) for r in routes},
                            "f+b": {r: fb(r) for r in routes if r != "gather" or has_gather_grad}}
                    ms = {(leg, r): [] for leg in legs for r in legs[leg]}
                    for n in range(WARMUP + ROUNDS):
                        for leg in legs:
                            for r in legs[leg]:
                                t = event_ms(legs[leg][r])
                                if n >= WARMUP:
                                    ms[leg, r].append(t)
                    peaks = {r: peak_mib(legs["fwd"][r]) for r in routes}
                    kern = kernels(fb("pool"))
                    elt = x.element_size()
                    for leg in legs:
                        med = {r: float(np.median(ms[leg, r])) for r in legs[leg]}
                        text = "  %-17s C=%-3d %s %-3s %-4s" % (name, c, label, red, leg)
                        text += "".join(" %s %s" % (r, cell(ms[leg, r])) for r in legs[leg])
                        text += "".join("  %s/pool %5.2fx" % (r, med[r] / med["pool"]) for r in legs[leg] if r != "pool")
                        if leg == "fwd":
                            text += "  peak MiB" + "".join(" %s %.0f" % (r, peaks[r]) for r in routes)
                        else:
                            arg = red == "max"
                            fname = "k_tpool_fwd<arg>" if arg else "k_tpool_fwd"
                            fbytes = model_bytes(rows, k, entries, c, elt, arg)
                            bbytes = v * 4 * k + entries * c * (elt + (2 if arg else 0)) + v * c * elt
                            text += "  kernel fwd %.3f ms = %.0f MB, %.0f%% of HBM peak; bwd %.3f ms = %.0f MB, %.0f%%" % (
                                kern[fname], fbytes / 1e6, 100 * fbytes / (kern[fname] * 1e-3) / HBM_PEAK,
                                kern["k_tpool_bwd"], bbytes / 1e6, 100 * bbytes / (kern["k_tpool_bwd"] * 1e-3) / HBM_PEAK)
                        lines.append(text)
                        print(text, flush=True)
            del x32, g32
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
