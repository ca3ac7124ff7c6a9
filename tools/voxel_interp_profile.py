"""VoxelInterp / voxel_interpolate (csrc/vnbr.hip's corner table, csrc/vinterp.hip) against the route a user had without them, on the 1
M-point LiDAR-like frame at the 704 x 800 x 40 grid -- the frame and the protocol of sparse_pool_profile.py: the sparse voxel features
interpolated back at ALL 1 M points of the cloud (trimmed points included).

  interp    VoxelInterp (the table build: three launches and one read-back), voxel_interpolate forward (one launch) and forward +
            backward (two launches; the inverted index is built once per frame, on the first backward: timed as "transpose")
  torch     linear keys over the box of the coordinates, ONE sort of the voxels' keys, eight searchsorted (one per corner),
            (feat[idx] * w[:, :, None]).sum(1) over a [K, 8, C] buffer (an absent corner reads the row the search stopped at, with
            weight 0), and one index_add_ (float atomics) of the PRESENT entries' products for the gradient: nothing is scattered for
            an absent corner, the list of present entries is made with the table

Timing: WARMUP untimed rounds, then ROUNDS rounds in which the variants alternate; HIP events around each call; median [min .. max]
in ms.  The results are compared before anything is timed.  peak: the most memory a call holds beyond what was allocated before it
(MiB).  kernel: the launch's own time (d3d_profile_report, a run of its own) and the bytes of the model of DESIGN.md 4d-5 over it, as a
fraction of the 8 TB/s HBM peak -- the gathered rows are counted once per present entry although most of those reads are served by
the caches.

usage: python tools/voxel_interp_profile.py [out.txt]   (writes profiles/voxel_interp_profile.txt by default)"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import _lib, synth                                                                  # noqa: E402
from d3d_amd.voxel import VoxelGenerator, VoxelInterp, voxel_interpolate, voxel_positions       # noqa: E402

WARMUP, ROUNDS = 3, 20
CHANNELS = (16, 64)
SHAPE = synth.KITTI_SHAPE
DTYPES = (("fp32", torch.float32), ("bf16", torch.bfloat16))
HBM_PEAK = 8e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


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


def torch_table(coords, pos):
    """-> (idx [K, 8] int64: the voxel's row, for an absent corner the row the search stopped at; w [K, 8], 0 where absent; present:
    the numbers of the present entries in the flattened table): the corner table from torch ops alone"""
    v = coords.shape[0]
    lo, hi = coords.min(0).values, coords.max(0).values
    span = hi - lo + 1
    keys = ((coords[:, 0] - lo[0]) * span[1] + (coords[:, 1] - lo[1])) * span[2] + (coords[:, 2] - lo[2])
    skeys, order = torch.sort(keys)
    b = torch.floor(pos)
    f = pos - b
    b = b.long()
    idx, w, hits = [], [], []
    for j in range(8):
        bits = torch.tensor([j >> 2 & 1, j >> 1 & 1, j & 1], device=pos.device)
        cc = b + bits
        inside = ((cc >= lo) & (cc <= hi)).all(1)
        rel = torch.where(inside[:, None], cc - lo, torch.zeros_like(cc))
        key = (rel[:, 0] * span[1] + rel[:, 1]) * span[2] + rel[:, 2]
        at = torch.searchsorted(skeys, key).clamp_(max=v - 1)
        hit = inside & (skeys[at] == key)
        wj = torch.where(bits.bool(), f, 1 - f).prod(1)
        idx.append(order[at])
        w.append(torch.where(hit, wj, torch.zeros_like(wj)))
        hits.append(hit)
    return torch.stack(idx, 1), torch.stack(w, 1), torch.nonzero(torch.stack(hits, 1).reshape(-1))[:, 0]


class TorchInterp(torch.autograd.Function):
    """(feat[idx] * w).sum over a [K, 8, C] buffer; the gradient by ONE index_add_ (float atomics) of the present entries' products"""

    @staticmethod
    def forward(ctx, x, idx, w, present):
        ctx.save_for_backward(idx, w, present)
        ctx.num_rows = x.shape[0]
        return (x[idx] * w[:, :, None].to(x.dtype)).sum(1)

    @staticmethod
    def backward(ctx, g):
        idx, w, present = ctx.saved_tensors
        out = g.new_zeros((int(ctx.num_rows), g.shape[1]))
        prod = (g[:, None, :] * w[:, :, None].to(g.dtype)).reshape(-1, g.shape[1])
        out.index_add_(0, idx.reshape(-1)[present], prod[present])
        return out, None, None, None


def torch_backward(x, table, g):
    a = x.detach().requires_grad_(True)
    TorchInterp.apply(a, *table).backward(g)
    return a.grad


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "voxel_interp_profile.txt")
    assert torch.cuda.is_available(), "voxel_interp_profile needs a GPU"
    torch.cuda.set_device(0)
    pts = torch.from_numpy(synth.lidar_like(1_000_000, 0)).cuda()
    gen = VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, max_points=32, max_points_filter="trim")
    coords = gen(pts).coords.long().contiguous()
    pos = voxel_positions(pts, gen._size.cuda(), gen._offset.cuda()).contiguous()
    v, k = coords.shape[0], pos.shape[0]
    itp = VoxelInterp(coords, pos)
    ttable = torch_table(coords, pos)
    idx, tw, present = ttable
    assert torch.equal(torch.nonzero(itp.table.view(-1) >= 0)[:, 0], present)
    assert torch.equal(itp.table.view(-1)[present].long(), idx.view(-1)[present])
    assert float((itp.weights - tw).abs().max()) <= 1e-6
    entries = itp.num_entries
    lines = ["%s; %d warm-up rounds, then per variant the median [min .. max] of %d timed rounds in ms, variants alternating inside a "
             "round, HIP events around each" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS),
             "lidar 1M: V = %d voxels, K = %d points, J = 8: %d entries present (%.2f per point, %.1f per voxel, %d in the most crowded "
             "voxel: the length of the longest sequential fold of the backward)" %
             (v, k, entries, entries / k, entries / v, int(itp.transpose().offsets.diff().max()))]
    print("\n".join(lines), flush=True)

    # ---- the table build
    builds = {"interp": lambda: VoxelInterp(coords, pos), "interp + transpose": lambda: VoxelInterp(coords, pos).transpose(),
              "torch": lambda: torch_table(coords, pos)}
    ms = {r: [] for r in builds}
    for n in range(WARMUP + ROUNDS):
        for r in builds:
            t = event_ms(builds[r])
            if n >= WARMUP:
                ms[r].append(t)
    peaks = {r: peak_mib(builds[r]) for r in builds}
    kern = kernels(builds["interp"])
    med = {r: float(np.median(ms[r])) for r in builds}
    text = "  table build (read-backs included)" + "".join("  %s %s" % (r, cell(ms[r])) for r in builds)
    text += "  torch/interp %5.2fx  torch/(interp + transpose) %5.2fx" % (med["torch"] / med["interp"], med["torch"] / med["interp + transpose"])
    text += "  peak MiB" + "".join(" %s %.0f" % (r, peaks[r]) for r in builds)
    text += "  kernels: bounds %.3f insert %.3f lookup %.3f ms; lookup = %.0f MB of positions, table and weights, %.0f%% of HBM peak" % (
        kern["k_vn_bounds"], kern["k_vn_insert"], kern["k_vc_lookup"], (k * 12 + k * 64) / 1e6,
        100 * (k * 12 + k * 64) / (kern["k_vc_lookup"] * 1e-3) / HBM_PEAK)
    lines.append(text)
    print(text, flush=True)
    itp.transpose()

    # ---- the operator
    for c in CHANNELS:
        x32 = torch.randn(v, c, device="cuda")
        g32 = torch.randn(k, c, device="cuda")
        for label, dt in DTYPES:
            x, g = x32.to(dt), g32.to(dt)
            routes = {"interp": lambda a: voxel_interpolate(a, itp), "torch": lambda a: TorchInterp.apply(a, *ttable)}

            def fb(r):
                def run():
                    a = x.detach().requires_grad_(True)
                    routes[r](a).backward(g)
                    return a.grad
                return run

            tol = 1e-4 if dt == torch.float32 else 0.05
            got, want = routes["interp"](x), routes["torch"](x)
            assert float((got.float() - want.float()).abs().max()) <= tol * float(want.float().abs().max()), (c, label)
            # (the gradient against the torch route in fp32: in bf16 its index_add_ rounds after every one of a crowded voxel's adds)
            a, b = fb("interp")(), torch_backward(x32, ttable, g.float())
            assert float((a.float() - b).abs().max()) <= tol * float(b.abs().max()), (c, label, "gradient")
            del got, want, a, b
            legs = {"fwd": {r: (lambda r=r: routes[r](x)) for r in routes}, "f+b": {r: fb(r) for r in routes}}
            ms = {(leg, r): [] for leg in legs for r in legs[leg]}
            for n in range(WARMUP + ROUNDS):
                for leg in legs:
                    for r in legs[leg]:
                        t = event_ms(legs[leg][r])
                        if n >= WARMUP:
                            ms[leg, r].append(t)
            peaks = {(leg, r): peak_mib(legs[leg][r]) for leg in legs for r in legs[leg]}
            kern = kernels(fb("interp"))
            elt = x.element_size()
            for leg in legs:
                med = {r: float(np.median(ms[leg, r])) for r in legs[leg]}
                text = "  C=%-3d %s %-4s" % (c, label, leg)
                text += "".join(" %s %s" % (r, cell(ms[leg, r])) for r in legs[leg])
                text += "  torch/interp %5.2fx" % (med["torch"] / med["interp"])
                text += "  peak MiB" + "".join(" %s %.0f" % (r, peaks[leg, r]) for r in legs[leg])
                if leg == "f+b":
                    fbytes = k * 8 * 8 + entries * c * elt + k * c * elt
                    bbytes = 8 * (v + 1) + entries * 8 + entries * c * elt + v * c * elt
                    kf, kb = kern["k_wfold<interp>"], kern["k_wfold<splat>"]
                    text += "  kernel fwd %.3f ms = %.0f MB, %.0f%% of HBM peak; bwd %.3f ms = %.0f MB, %.0f%%" % (
                        kf, fbytes / 1e6, 100 * fbytes / (kf * 1e-3) / HBM_PEAK, kb, bbytes / 1e6, 100 * bbytes / (kb * 1e-3) / HBM_PEAK)
                lines.append(text)
                print(text, flush=True)
        del x32, g32
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
