"""FrustumMap / lift_splat (csrc/vlift.hip) against the two routes a user had without them, at the shapes of two camera BEV detectors.

  shapes    bevfusion  B 1, N 6, D 118, 32 x 88, C 80, grid 360 x 360 x 1 (0.3 m cells over +-54 m)
            bevdet     B 1, N 6, D 59, 16 x 44, C 64, grid 128 x 128 x 1 (0.8 m cells over +-51.2 m)
            six pinhole cameras in a ring (1266 px focal length, 1600 x 900 resized by 0.48 and cropped to 704 x 256), depth bins from 1 m
  map       FrustumMap (count, read-back, emit, VoxelIndex and its read-back) against the same geometry in torch: the affine maps, the
            division, .long(), the mask, torch.unique(return_inverse) for the numbering
  lift      lift_splat forward (one launch) and forward + backward in depth and feat (three launches)
  index_add the materialised product depth[..., None] * feat [K, C], its kept rows, zeros(V, C).index_add_ (float atomics: LSS without
            the cumsum trick); the kept rows' indices are precomputed, as the map is for lift
  pool      the same product into this library's voxel_pool(sum) through the map's VoxelIndex

Timing: WARMUP untimed rounds, then ROUNDS rounds in which the variants alternate; HIP events around each call; median [min .. max] in
ms.  The results are compared before anything is timed (lift == pool bit for bit in fp32; index_add within a tolerance: its order is
not defined).  peak: torch.cuda.max_memory_allocated over one call, above what was allocated before it.  The baseline of a leg is the
FASTER torch-side route; a leg that does not beat it is marked LOSES.  kernel: the launch's own time (d3d_profile_report, a run of its
own) and its model bytes over it as a share of the 8 TB/s HBM peak --
  forward         M (4 + s) of order and depth + S H W C s of feature rows (each read once: the M C s of gathered rows hit the caches
                  where a cell's points share pixels) + V C s stored + 8 (V + 1)
  backward_feat   K (8 + s) of mapping and depth + V C s of gradient rows + S H W C s stored
  backward_depth  K 8 of mapping + S H W C s + V C s + K s stored
(M the members, s the element size) -- and the longest fold: the points of the most crowded cell, which one lane group walks in order.

usage: python tools/lift_profile.py [out.txt]   (writes profiles/lift_profile.txt by default)"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import _lib                                                                          # noqa: E402
from d3d_amd.voxel import FrustumMap, frustum_matrices, lift_splat, voxel_pool                   # noqa: E402

WARMUP, ROUNDS = 3, 20
DTYPES = (("fp32", torch.float32), ("bf16", torch.bfloat16))
HBM_PEAK = 8e12
SHAPES = (("bevfusion", 118, 32, 88, 80, (-54, 54, -54, 54, -10, 10), (360, 360, 1), np.arange(118) * 0.5 + 1.0),
          ("bevdet", 59, 16, 44, 64, (-51.2, 51.2, -51.2, 51.2, -5, 3), (128, 128, 1), np.arange(59) * 1.0 + 1.0))
CAMS = 6
# variants that were tried on these two shapes (fp32, the launch's own time in ms, bevfusion / bevdet) -- measured once each, when tried;
# the code of the dropped ones is gone
TRIED = (
    "variants tried (fp32 kernel ms, bevfusion / bevdet; measured once each when tried):",
    "  k_lift_fwd, four rows in flight, the pixel by two 32-bit divisions per entry: 0.154 / -; with the next step's `order` entries "
    "fetched under the rows: 0.157 / 0.078 (no gain on its own: the entries of a step share a cache line with the last step's; kept, "
    "it was not measured again alone after the next change)",
    "  k_lift_fwd, the pixel by multiplication (Granlund-Montgomery) instead: 0.125 / 0.055 -- KEPT: the launch waits for the most "
    "crowded cell's lane group, whose time is its instruction stream",
    "  k_lift_fwd, eight rows in flight: 0.102 / 0.049 -- KEPT;  k_lift_bwd_feat, eight depth bins in flight: 0.133 / 0.020 against "
    "0.106 / 0.021 with four -- DROPPED (it stays at four)",
    "  k_fm_cells, an agent-scope load of the bitmap word before the atomic OR (skip it when the bit is set): 0.478 against 0.378 / "
    "0.140 against 0.140 -- DROPPED: the look is another trip to L2 for every point",
)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cell(x):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(x)), min(x), max(x))


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


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


def calibrations():
    """six cameras in a ring: (pre, post) [6, 3, 4] float32"""
    yaw = np.arange(CAMS) * (2 * np.pi / CAMS)
    c, s = np.cos(yaw), np.sin(yaw)
    turn = np.zeros((CAMS, 3, 3))
    turn[:, 0, 0], turn[:, 0, 1], turn[:, 1, 0], turn[:, 1, 1], turn[:, 2, 2] = c, -s, s, c, 1
    rots = turn @ np.array([[0, 0, 1.0], [-1, 0, 0], [0, -1, 0]])                 # the camera looks along its z, x right, y down
    trans = np.stack([1.5 * c, 1.5 * s, np.full(CAMS, 1.5)], 1)
    intrins = np.broadcast_to(np.array([[1266.0, 0, 816], [0, 1266.0, 491], [0, 0, 1]]), (CAMS, 3, 3)).copy()
    post_rots = np.broadcast_to(np.diag([0.48, 0.48, 1.0]), (CAMS, 3, 3)).copy()
    post_trans = np.broadcast_to(np.array([-32.0, -176.0, 0]), (CAMS, 3)).copy()
    return frustum_matrices(rots, trans, intrins, post_rots, post_trans)


def torch_map(us, vs, ds, pre, post, lo, size, shape):
    """the geometry in torch: -> (rows of the kept points, their indices, coords)"""
    a = torch.stack(torch.meshgrid(ds, vs, us, indexing="ij")[::-1], -1)                              # [D, H, W, 3] = (u, v, d)
    q = torch.einsum("sij,dhwj->sdhwi", pre[:, :, :3], a) + pre[:, None, None, None, :, 3]
    e = torch.cat([q[..., :2] * q[..., 2:3], q[..., 2:3]], -1)
    x = torch.einsum("sij,sdhwj->sdhwi", post[:, :, :3], e) + post[:, None, None, None, :, 3]
    t = ((x - lo) / size).reshape(-1, 3)
    kept = ((t >= 0) & (t < shape)).all(1)
    c = t[kept].long()
    key = (c[:, 0] * int(shape[1]) + c[:, 1]) * int(shape[2]) + c[:, 2]
    uniq, rows = torch.unique(key, return_inverse=True)
    return rows, kept.nonzero().squeeze(1), uniq


def leg(lines, title, d, h, w, c, bounds, shape, ds):
    us, vs = np.linspace(0, 703, w).astype(np.float32), np.linspace(0, 255, h).astype(np.float32)
    ds = ds.astype(np.float32)
    pre, post = calibrations()
    args = (us, vs, ds, pre, post, bounds, shape, CAMS)
    fmap = FrustumMap(*args)
    s, k, v, m = CAMS, fmap.num_points, fmap.num_voxels, fmap.num_members
    dev = [torch.from_numpy(x).cuda() for x in (us, vs, ds, pre, post, fmap.lo, fmap.size)] + [torch.tensor(shape, device="cuda").float()]
    # the torch routes fold through the map's own rows; torch's geometry (einsum may fuse, its rounding is not the contract's) is timed
    # and its disagreement counted, not used
    kept_idx = (fmap.mapping >= 0).nonzero().squeeze(1)
    rows = fmap.mapping[kept_idx]
    t_rows, t_kept, t_uniq = torch_map(*dev)
    differ = kept_idx.numel() != t_kept.numel() or not torch.equal(kept_idx, t_kept) or not torch.equal(rows, t_rows)
    differ = int((torch.zeros(k, dtype=torch.int64, device="cuda").index_put_((t_kept,), t_rows + 1) != fmap.mapping + 1).sum()) if differ else 0
    ms = {"map": [], "torch map": []}
    for i in range(WARMUP + ROUNDS):
        for name, fn in (("map", lambda: FrustumMap(*args)), ("torch map", lambda: torch_map(*dev))):
            t = event_ms(fn)
            if i >= WARMUP:
                ms[name].append(t)
    longest = int(torch.diff(fmap.index.offsets).max()) if v else 0
    med = {n: float(np.median(x)) for n, x in ms.items()}
    text = "%s: S = %d cameras, D = %d, %d x %d, C = %d, grid %s: K = %d points, %d members (%.1f %%), V = %d cells present, longest fold %d points" % (
        title, s, d, h, w, c, "x".join(map(str, shape)), k, m, 100.0 * m / k, v, longest)
    lines.append(text)
    print(text, flush=True)
    text = "  map build (read-backs included) %s  torch geometry + unique %s  torch/map %5.2fx%s; peak %.1f MB against %.1f MB" % (
        cell(ms["map"]), cell(ms["torch map"]), med["torch map"] / med["map"], "" if med["map"] < med["torch map"] else "  LOSES",
        peak_of(lambda: FrustumMap(*args)) / 1e6, peak_of(lambda: torch_map(*dev)) / 1e6)
    kern = kernels(lambda: FrustumMap(*args))
    text += "; %d points land elsewhere under torch's rounding; launches " % differ + ", ".join("%s %.3f" % (n, kern[n]) for n in sorted(kern))
    lines.append(text)
    print(text, flush=True)
    gen = torch.Generator().manual_seed(0)
    depth32 = torch.rand((s, d, h, w), generator=gen).cuda().softmax(1)
    feat32 = torch.randn((s, h, w, c), generator=gen).cuda()
    grad32 = torch.randn((v, c), generator=gen).cuda()
    for label, dt in DTYPES:
        depth, feat, grad = depth32.to(dt), feat32.to(dt), grad32.to(dt)

        def product(a, b):
            return (a[..., None] * b[:, None]).reshape(k, c)
        routes = {"lift": lambda a, b: lift_splat(a, b, fmap),
                  "index_add": lambda a, b: a.new_zeros((v, c)).index_add_(0, rows, product(a, b)[kept_idx]),
                  "pool": lambda a, b: voxel_pool(product(a, b), fmap.index, reduction="sum")}
        if dt != torch.float32:
            del routes["pool"]                                   # (voxel_pool is fp32 / fp64 only)

        def fb(r):
            def run():
                a, b = depth.detach().requires_grad_(True), feat.detach().requires_grad_(True)
                routes[r](a, b).backward(grad)
                return a.grad, b.grad
            return run

        got = routes["lift"](depth, feat)
        if "pool" in routes:
            assert torch.equal(got, routes["pool"](depth, feat)), (title, label, "lift != pool")
        # (against index_add_ in fp32 on the same values: in bf16 its own atomic sums of hundreds of rows are too coarse to check with)
        a32, b32 = depth.float().clone().requires_grad_(True), feat.float().clone().requires_grad_(True)
        loose = routes["index_add"](a32, b32)
        loose.backward(grad.float())
        tol = 1e-4 if dt == torch.float32 else 2.0 ** -7
        for x, y, what in zip((got,) + fb("lift")(), (loose.detach(), a32.grad, b32.grad), ("forward", "grad_depth", "grad_feat")):
            assert torch.allclose(x.float(), y, rtol=tol, atol=tol * float(y.abs().max())), (title, label, what)
        del got, loose, a32, b32
        legs = {"fwd": {r: (lambda r=r: routes[r](depth, feat)) for r in routes}, "f+b": {r: fb(r) for r in routes}}
        ms = {(kk, r): [] for kk in legs for r in legs[kk]}
        for i in range(WARMUP + ROUNDS):
            for kk in legs:
                for r in legs[kk]:
                    t = event_ms(legs[kk][r])
                    if i >= WARMUP:
                        ms[kk, r].append(t)
        kern = kernels(fb("lift"))
        e = depth.element_size()
        model = {"k_lift_fwd": m * (4 + e) + s * h * w * c * e + v * c * e + 8 * (v + 1),
                 "k_lift_bwd_feat": k * (8 + e) + v * c * e + s * h * w * c * e,
                 "k_lift_bwd_depth": k * 8 + s * h * w * c * e + v * c * e + k * e}
        for kk in legs:
            med = {r: float(np.median(ms[kk, r])) for r in legs[kk]}
            base = min((r for r in routes if r != "lift"), key=lambda r: med[r])
            text = "  %s %-4s" % (label, kk) + "".join(" %s %s" % (r, cell(ms[kk, r])) for r in legs[kk])
            text += "  baseline %s, baseline/lift %5.2fx%s" % (base, med[base] / med["lift"], "" if med["lift"] < med[base] else "  LOSES")
            text += "  peak MB " + " ".join("%s %.1f" % (r, peak_of(legs[kk][r]) / 1e6) for r in legs[kk])
            lines.append(text)
            print(text, flush=True)
        text = "  %s kernels " % label + "; ".join("%s %.3f ms = %.1f MB, %.1f%% of HBM peak" % (
            n, kern[n], model[n] / 1e6, 100 * model[n] / (kern[n] * 1e-3) / HBM_PEAK) for n in model)
        text += "; the longest fold of %d points: %.0f ns per point if it alone set k_lift_fwd's time" % (
            longest, kern["k_lift_fwd"] * 1e6 / max(longest, 1))
        lines.append(text)
        print(text, flush=True)
        del depth, feat, grad
        torch.cuda.empty_cache()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lift_profile.txt")
    assert torch.cuda.is_available(), "lift_profile needs a GPU"
    torch.cuda.set_device(0)
    lines = ["%s; %d warm-up rounds, then per variant the median [min .. max] of %d timed rounds in ms, variants alternating inside a "
             "round, HIP events around each" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS)]
    print(lines[0], flush=True)
    for shape in SHAPES:
        leg(lines, *shape)
    lines.extend(TRIED)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
