"""voxel_to_dense (csrc/vdense.hip) against the two routes a user had without it, on the 1 M-point LiDAR-like frame -- the frame and
the protocol of voxel_interp_profile.py.

  legs      bev     the frame taken through three k3 s2 p1 SparseConvMaps to the 88 x 100 x 5 grid, C = 128, as [N, C, Z, Y, X];
                    batch 1 and batch 4 (the same frame under four batch values)
            stage1  the first-stage 704 x 800 x 40 grid at C = 16: nearly all of the time is the fill
  dense     voxel_to_dense forward (one launch) and forward + backward (two launches); the VoxelDenseMap is built once per frame
            and stage and is timed on its own
  spconv    torch.zeros [N, Z, Y, X, C], index_put_, permute(0, 4, 1, 2, 3).contiguous(): spconv's .dense()
  direct    torch.zeros [N, C, Z, Y, X], index_put_ through (n, :, z, y, x)
  full      torch.full of the output's size alone: the store floor

Timing: WARMUP untimed rounds, then ROUNDS rounds in which the variants alternate; HIP events around each call; median [min .. max]
in ms.  The results are compared (bit for bit) before anything is timed.  The baseline of a leg is the FASTER torch route; a leg
that does not beat it is marked LOSES.  kernel: the launch's own time (d3d_profile_report, a run of its own) and the model bytes
N C P s + V C s + 4 N P over it, as a fraction of the 8 TB/s HBM peak.

usage: python tools/voxel_dense_profile.py [out.txt]   (writes profiles/voxel_dense_profile.txt by default)"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import _lib, synth                                                                  # noqa: E402
from d3d_amd.voxel import SparseConvMap, VoxelDenseMap, VoxelGenerator, voxel_to_dense          # noqa: E402

WARMUP, ROUNDS = 3, 20
SHAPE = synth.KITTI_SHAPE
DTYPES = (("fp32", torch.float32), ("bf16", torch.bfloat16))
HBM_PEAK = 8e12
AXES = (2, 1, 0)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cell(x):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(x)), min(x), max(x))


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


def spconv_route(x, at, n, dshape):
    grid = x.new_zeros((n,) + dshape + (x.shape[1],)).index_put_(at, x)
    return grid.permute(0, 4, 1, 2, 3).contiguous()


def direct_route(x, at, n, dshape):
    out = x.new_zeros((n, x.shape[1]) + dshape)
    out[at[0], :, at[1], at[2], at[3]] = x
    return out


def leg(lines, title, coords, batch, n, shape, c):
    dshape = tuple(shape[a] for a in AXES)
    v, p = coords.shape[0], shape[0] * shape[1] * shape[2]
    dmap = VoxelDenseMap(coords, shape, batch_index=batch, batch_size=None if batch is None else n, axes=AXES)
    build = [event_ms(lambda: VoxelDenseMap(coords, shape, batch_index=batch, batch_size=None if batch is None else n, axes=AXES))
             for _ in range(WARMUP + ROUNDS)][WARMUP:]
    at = (torch.zeros(v, dtype=torch.int64, device="cuda") if batch is None else batch,) + tuple(coords[:, a].contiguous() for a in AXES)
    lib = _lib.load()
    tile, sparse = lib.d3d_vdense_tile_cells(), lib.d3d_vdense_sparse_cells()
    per = torch.nn.functional.pad((dmap.index >= 0).view(n, p), (0, -p % tile)).view(-1, tile).sum(1)      # present cells per stretch
    text = "%s: V = %d voxels, N = %d, grid %s (P = %d cells, %.1f %% present), C = %d; map build (read-back included) %s" % (
        title, v, n, "x".join(map(str, dshape)), p, 100.0 * v / (n * p), c, cell(build))
    text += "; %d stretches of %d cells: %d empty, %d sparse (1 .. %d present), %d through the tile" % (
        per.numel(), tile, int((per == 0).sum()), int(((per > 0) & (per <= sparse)).sum()), sparse, int((per > sparse).sum()))
    lines.append(text)
    print(text, flush=True)
    x32 = torch.randn(v, c, device="cuda")
    for label, dt in DTYPES:
        x = x32.to(dt)
        g = torch.randn((n, c) + dshape, device="cuda", dtype=dt)
        routes = {"dense": lambda a: voxel_to_dense(a, dmap), "spconv": lambda a: spconv_route(a, at, n, dshape),
                  "direct": lambda a: direct_route(a, at, n, dshape)}

        def fb(r):
            def run():
                a = x.detach().requires_grad_(True)
                routes[r](a).backward(g)
                return a.grad
            return run

        want, want_grad = routes["spconv"](x), fb("spconv")()
        for r in ("dense", "direct"):
            assert torch.equal(routes[r](x), want) and torch.equal(fb(r)(), want_grad), (title, label, r)
        del want, want_grad
        legs = {"fwd": {r: (lambda r=r: routes[r](x)) for r in routes}, "f+b": {r: fb(r) for r in routes}}
        legs["fwd"]["full"] = lambda: torch.full((n, c) + dshape, 1.5, device="cuda", dtype=dt)
        ms = {(k, r): [] for k in legs for r in legs[k]}
        for i in range(WARMUP + ROUNDS):
            for k in legs:
                for r in legs[k]:
                    t = event_ms(legs[k][r])
                    if i >= WARMUP:
                        ms[k, r].append(t)
        kern = kernels(fb("dense"))
        elt = x.element_size()
        model = n * c * p * elt + v * c * elt + 4 * n * p
        for k in legs:
            med = {r: float(np.median(ms[k, r])) for r in legs[k]}
            base = min(("spconv", "direct"), key=lambda r: med[r])
            text = "  %s %-4s" % (label, k) + "".join(" %s %s" % (r, cell(ms[k, r])) for r in legs[k])
            text += "  baseline %s, baseline/dense %5.2fx%s" % (base, med[base] / med["dense"], "" if med["dense"] < med[base] else "  LOSES")
            if k == "fwd":
                text += "  dense/full %4.2f" % (med["dense"] / med["full"])
            else:
                ks, kg = kern["k_vdense<scatter>"], kern["k_vdense<gather>"]
                text += "  kernel scatter %.3f ms = %.0f MB, %.0f%% of HBM peak; gather %.3f ms" % (ks, model / 1e6, 100 * model / (ks * 1e-3) / HBM_PEAK, kg)
            lines.append(text)
            print(text, flush=True)
        del x, g
        torch.cuda.empty_cache()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "voxel_dense_profile.txt")
    assert torch.cuda.is_available(), "voxel_dense_profile needs a GPU"
    torch.cuda.set_device(0)
    pts = torch.from_numpy(synth.lidar_like(1_000_000, 0)).cuda()
    gen = VoxelGenerator(synth.KITTI_BOUNDS, SHAPE, max_points=32, max_points_filter="trim")
    first = gen(pts).coords.long().contiguous()
    coords, shape = first, tuple(SHAPE)
    for _ in range(3):
        cmap = SparseConvMap(coords, 3, 2, 1, spatial_shape=shape)
        coords, shape = cmap.out_coords, tuple((s + 2 - 3) // 2 + 1 for s in shape)
    lines = ["%s; %d warm-up rounds, then per variant the median [min .. max] of %d timed rounds in ms, variants alternating inside a "
             "round, HIP events around each" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS)]
    print(lines[0], flush=True)
    leg(lines, "bev batch 1", coords, None, 1, shape, 128)
    four = coords.repeat(4, 1)
    batch = torch.arange(4, device="cuda").repeat_interleave(coords.shape[0])
    leg(lines, "bev batch 4", four, batch, 4, shape, 128)
    leg(lines, "stage1", first, None, 1, tuple(SHAPE), 16)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
