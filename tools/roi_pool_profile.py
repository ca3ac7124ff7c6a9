"""RoiGrid and roiaware_pool3d (csrc/roipool.hip, csrc/vtpool.hip) against what a user had without them: torch alone.

  shapes        128 and 512 boxes of car size centred on points of the cloud, 12^3 cells, P = 128; a 16 384-point keypoint set and a
                150 000-point frame; C = 16 and 128; fp32 and bf16
  legs          the table build (its m * G * P slots of padding are stored by the same launch and counted in the time), transpose()
                once, the pooling forward (max), forward + backward, and the peak memory of every leg
  torch         pairwise local coordinates [slab of boxes, N] -> mask -> nonzero -> cell keys (its "table": a list of (cell, point)
                pairs, uncapped); pooling: feat[point] gathered and scatter_reduce_(amax) into [M * G, C] -- float atomics -- and its
                autograd.  Same process, same boxes.
  Every figure measured is written down with the peak memory of the leg; a leg where the kernel is slower is marked LOSES.

Timing: WARMUP untimed rounds, then ROUNDS timed ones, HIP events around each call, median [min .. max] in ms.  Results are compared
before anything is timed and the outcome is written next to the numbers: the share of cells whose pooled row is equal (the torch
route does not cap a cell at P and takes its sine and cosine from torch, so a few cells may differ).

usage: python tools/roi_pool_profile.py [out.txt]   (writes profiles/roi_pool_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                              # noqa: E402
from d3d_amd.point import RoiGrid, roiaware_pool3d                     # noqa: E402

WARMUP, ROUNDS = 2, 7

# Recorded ONCE, with code that is no longer in the library: the first k_roi_grid cut the WHOLE segment into 8 slabs, one per
# wavefront, queued up to 256 members per slab, let wavefront 0 alone place all queues (peeling one cell at a time) and walked a slab
# a second time where its queue overflowed.  Same tables, same tests; on a 150 000-point frame a box near the sensor holds thousands
# of points, every queue overflows, and one wavefront walks the frame again and places every member: the launch lasts as long as its
# most crowded box.  Rounds of 256-row slabs (a queue holds a whole slab: no overflow, no second walk) and placing by the wavefront
# that owns the cell replaced it.  This tool copies the block to the end of the file.
VARIANT_AB = """
A/B of the table kernel's first variant, recorded once (not kept: slabs over the whole segment, one wavefront placing, a second walk where a slab's queue of 256 overflows; table build only, same shapes, same process as its torch column):
keypoints N  16384 M 128  first variant     0.346 [    0.339 ..     0.352] ms   torch     0.272 ms   torch/variant   0.78x  LOSES
keypoints N  16384 M 512  first variant     0.355 [    0.352 ..     0.358] ms   torch     0.619 ms   torch/variant   1.74x
frame     N 150000 M 128  first variant     4.044 [    4.005 ..     4.113] ms   torch     1.330 ms   torch/variant   0.33x  LOSES
frame     N 150000 M 512  first variant     3.847 [    3.837 ..     3.880] ms   torch     5.396 ms   torch/variant   1.40x
"""
OUT, P = 12, 128
G = OUT ** 3
SLAB = 2 ** 26                     # pairs (box, point) a torch leg holds at a time


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, rounds=ROUNDS):
    """-> (times in ms, peak bytes allocated while they ran)"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times = [event_ms(fn) for _ in range(rounds)]
    return times, torch.cuda.max_memory_allocated() - base


def cell(x):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(x)), min(x), max(x))


def mib(b):
    return "%8.1f MiB" % (b / 2 ** 20)


OUT_PATH = [None]


def emit(lines, text):
    """every line goes to the file at once: a run that is cut short leaves what it measured"""
    lines.append(text)
    print(text, flush=True)
    if OUT_PATH[0]:
        with open(OUT_PATH[0], "w") as fo:
            fo.write("\n".join(lines) + "\n")


def verdict(lines, what, t_ours, m_ours, t_torch, m_torch, note=""):
    mo, mt = float(np.median(t_ours)), float(np.median(t_torch))
    emit(lines, "  %-20s ours %s ms (peak %s)   torch %s ms (peak %s)   torch/ours %6.2fx%s%s"
         % (what, cell(t_ours), mib(m_ours), cell(t_torch), mib(m_torch), mt / mo, "" if mo < mt else "  LOSES", note))


def torch_pairs(points, boxes):
    """-> (key [E] int64 = box * G + cell, point [E] int64): the torch-only route to "which point lies in which cell", uncapped"""
    xyz = points[:, :3]
    keys, rows = [], []
    step = max(1, SLAB // max(1, xyz.shape[0]))
    for a in range(0, boxes.shape[0], step):
        b = boxes[a:a + step]
        d = xyz[None, :, :] - b[:, None, :3]
        c, s = torch.cos(b[:, 6])[:, None], torch.sin(b[:, 6])[:, None]
        u, v = d[..., 0] * c + d[..., 1] * s, d[..., 1] * c - d[..., 0] * s
        t = torch.stack([u / b[:, None, 3], v / b[:, None, 4], d[..., 2] / b[:, None, 5]], -1) + 0.5
        bi, pi = torch.nonzero(((t >= 0) & (t <= 1)).all(-1), as_tuple=True)
        idx = (t[bi, pi] * OUT).long().clamp_(0, OUT - 1)
        keys.append((bi + a) * G + (idx[:, 0] * OUT + idx[:, 1]) * OUT + idx[:, 2])
        rows.append(pi)
    return torch.cat(keys), torch.cat(rows)


def torch_pool(feat, keys, rows, m):
    out = torch.zeros((m * G, feat.shape[1]), dtype=feat.dtype, device=feat.device)
    return out.scatter_reduce(0, keys[:, None].expand(-1, feat.shape[1]), feat[rows], "amax", include_self=False)


def frame(lines, name, points, m):
    n = points.shape[0]
    rng = np.random.default_rng(m)
    centres = points[torch.from_numpy(rng.choice(n, m, replace=False)).cuda(), :3]
    size = torch.tensor([4.2, 1.8, 1.6], device="cuda") * torch.from_numpy(rng.uniform(0.9, 1.1, (m, 3)).astype(np.float32)).cuda()
    boxes = torch.cat([centres, size, torch.from_numpy(rng.uniform(-3.1, 3.1, (m, 1)).astype(np.float32)).cuda()], 1).contiguous()
    grid = RoiGrid(points, boxes, OUT, P)
    keys, rows = torch_pairs(points, boxes)
    members, kept = int(grid.inside.sum()), int(grid.counts.sum())
    emit(lines, "%s: N %d points, M %d boxes, %d^3 cells, P %d: %d members (%d kept; the torch route finds %d), table %s"
         % (name, n, m, OUT, P, members, kept, keys.numel(), mib(grid.table.numel() * 4)))
    t_ours, m_ours = timed(lambda: RoiGrid(points, boxes, OUT, P))
    t_torch, m_torch = timed(lambda: torch_pairs(points, boxes))
    verdict(lines, "table build", t_ours, m_ours, t_torch, m_torch,
            "   (ours stores %.0f MB of slots, %.0f GB/s)" % (grid.table.numel() * 4 / 1e6, grid.table.numel() * 4 / np.median(t_ours) / 1e6))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t_once = event_ms(grid.transpose)
    emit(lines, "  %-20s ours %9.3f ms, once per grid (peak %s): nonzero over the table, d3d_voxel_index over the %d present entries"
         % ("transpose()", t_once, mib(torch.cuda.max_memory_allocated() - base), kept))
    for dtype in (torch.float32, torch.bfloat16):
        for c in (16, 128):
            gen = torch.Generator().manual_seed(c)
            feat = torch.randn((n, c), generator=gen).to(dtype).cuda().requires_grad_()
            grad = torch.randn((m * G, c), generator=gen).to(dtype).cuda()
            ours, theirs = roiaware_pool3d(feat, grid, "max").view(m * G, c), torch_pool(feat, keys, rows, m)
            same = float((ours == theirs).all(1).float().mean())
            g_ours, = torch.autograd.grad(ours, feat, grad)
            g_theirs, = torch.autograd.grad(theirs, feat, grad)
            gsame = float((g_ours == g_theirs).all(1).float().mean())
            emit(lines, " C %3d %-8s cells equal to torch's %.4f, gradient rows equal %.4f" % (c, str(dtype).replace("torch.", ""), same, gsame))

            def fwd_ours():
                return roiaware_pool3d(feat, grid, "max")

            def fwd_torch():
                return torch_pool(feat, keys, rows, m)

            def both(fn):
                def run():
                    torch.autograd.grad(fn().view(m * G, c), feat, grad)
                return run

            for what, f_ours, f_torch in (("forward", fwd_ours, fwd_torch), ("forward + backward", both(fwd_ours), both(fwd_torch))):
                t_ours, m_ours = timed(f_ours)
                t_torch, m_torch = timed(f_torch)
                verdict(lines, what, t_ours, m_ours, t_torch, m_torch)
    del grid, keys, rows
    torch.cuda.empty_cache()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "roi_pool_profile.txt")
    assert torch.cuda.is_available(), "roi_pool_profile needs a GPU"
    torch.cuda.set_device(0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    OUT_PATH[0] = out_path
    lines = []
    emit(lines, "%s; %d warm-up rounds, then the median [min .. max] of %d timed rounds in ms, HIP events around each call; peak = bytes "
         "allocated above the leg's inputs while it was timed" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS))
    emit(lines, "table build: one workgroup per box walks its whole segment, O(M N) by design, and stores every slot of [M, G, P]; the torch "
         "route builds [boxes, N] local coordinates (in slabs of 2^26 pairs) and keeps (cell, point) pairs, uncapped")
    keypoints = torch.from_numpy(synth.lidar_like(16384, 3)).cuda()
    cloud = torch.from_numpy(synth.lidar_like(150000, 4)).cuda()
    for name, pts in (("keypoints", keypoints), ("frame", cloud)):
        for m in (128, 512):
            frame(lines, name, pts, m)
    for text in VARIANT_AB.strip("\n").splitlines():
        emit(lines, text)


if __name__ == "__main__":
    main()
