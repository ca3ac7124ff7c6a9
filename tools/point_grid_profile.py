"""The grid routes of ball_query and knn_query (PointGrid; csrc/pgrid.hip) against the brute-force routes of the same commit
(csrc/psample.hip), on the same GPU in the same process.

  whole frame   100 000 x 100 000 rows of a LiDAR-like frame against themselves: ball r 0.8 nsample 16 / 32, kNN k 3 / 16
  keypoints     2048 FPS samples of 150 000 and of 16 384 rows, ball r 0.8 nsample 16 / 32 (what the brute-force route was made for)
  uniform       100 000 rows uniform in a box, and the same rows sorted along x (the brute-force walk ends early on neither)
  build         PointGrid alone: bounds, the read-back, the plan, the index, the packed coordinates
  A grid leg is the QUERY on a grid built before; "with build" adds the build's median.  Every figure measured is written down; a leg
  where the grid route is slower than the brute-force route is marked LOSES (with and without the build).

Timing: WARMUP untimed rounds, then ROUNDS timed ones, HIP events around each call, median [min .. max] in ms.  The two routes'
results are compared bit for bit before anything is timed and the outcome is written next to the numbers.

usage: python tools/point_grid_profile.py [out.txt]   (writes profiles/point_grid_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                                   # noqa: E402
from d3d_amd.point import PointGrid, ball_query, furthest_point_sample, knn_query           # noqa: E402

WARMUP, ROUNDS = 2, 10


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    return [event_ms(fn) for _ in range(ROUNDS)]


def cell(x):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(x)), min(x), max(x))


def emit(lines, text):
    lines.append(text)
    print(text, flush=True)


def verdict(grid_ms, brute_ms):
    return "brute/grid %6.2fx%s" % (brute_ms / grid_ms, "" if grid_ms < brute_ms else "  LOSES")


def build_leg(lines, name, pts, cell_size):
    t = timed(lambda: PointGrid(pts, cell_size))
    grid = PointGrid(pts, cell_size)
    emit(lines, "build %-26s N %6d cell %.2f -> %s, %d cells (h %.2f)   %s ms" % (name, pts.shape[0], cell_size, "x".join(str(d) for d in grid.dims[0]),
                                                                                grid.num_cells, grid.cell_size[0], cell(t)))
    return grid, float(np.median(t))


def ball_leg(lines, name, pts, grid, build_ms, ctr, r, nsample):
    got, want = ball_query(grid, ctr, r, nsample), ball_query(pts, ctr, r, nsample)
    same = torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    tg, tb = timed(lambda: ball_query(grid, ctr, r, nsample)), timed(lambda: ball_query(pts, ctr, r, nsample))
    mg, mb = float(np.median(tg)), float(np.median(tb))
    emit(lines, "ball %-27s M %6d x N %6d r %.1f nsample %2d  grid %s ms   brute force %s ms   %s   with build %8.3f ms: %s   same bits: %s   "
         "mean count %.1f" % (name, ctr.shape[0], pts.shape[0], r, nsample, cell(tg), cell(tb), verdict(mg, mb), mg + build_ms,
                              verdict(mg + build_ms, mb), same, float(got[1].float().mean())))


def knn_leg(lines, name, pts, grid, build_ms, ctr, k):
    got, want = knn_query(grid, ctr, k), knn_query(pts, ctr, k)
    same = torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    tg, tb = timed(lambda: knn_query(grid, ctr, k)), timed(lambda: knn_query(pts, ctr, k))
    mg, mb = float(np.median(tg)), float(np.median(tb))
    emit(lines, "knn  %-27s M %6d x N %6d k %2d               grid %s ms   brute force %s ms   %s   with build %8.3f ms: %s   same bits: %s"
         % (name, ctr.shape[0], pts.shape[0], k, cell(tg), cell(tb), verdict(mg, mb), mg + build_ms, verdict(mg + build_ms, mb), same))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "point_grid_profile.txt")
    assert torch.cuda.is_available(), "point_grid_profile needs a GPU"
    torch.cuda.set_device(0)
    lines = []
    emit(lines, "%s; %d warm-up rounds, then the median [min .. max] of %d timed rounds in ms, HIP events around each call (Python front included); "
         "both routes in this process, results compared bit for bit first" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS))
    frame = torch.from_numpy(synth.lidar_like(100000, 4)).cuda()
    grid, b = build_leg(lines, "LiDAR-like frame", frame, 0.8)
    for nsample in (16, 32):
        ball_leg(lines, "whole frame", frame, grid, b, frame, 0.8, nsample)
    for k in (3, 16):
        knn_leg(lines, "whole frame", frame, grid, b, frame, k)
    fine, bf = build_leg(lines, "LiDAR-like frame, fine", frame, 0.4)
    knn_leg(lines, "whole frame, cells of 0.4", frame, fine, bf, frame, 3)
    for n in (150000, 16384):
        cloud = torch.from_numpy(synth.lidar_like(n, 5)).cuda()
        keys = cloud[furthest_point_sample(cloud, 2048)].contiguous()
        grid, b = build_leg(lines, "keypoint cloud", cloud, 0.8)
        for nsample in (16, 32):
            ball_leg(lines, "2048 keypoints", cloud, grid, b, keys, 0.8, nsample)
    gen = torch.Generator().manual_seed(7)
    uniform = (torch.rand((100000, 3), generator=gen) * torch.tensor([80.0, 80.0, 4.0])).cuda()
    ordered = uniform[uniform[:, 0].argsort()].contiguous()
    for name, pts in (("uniform box", uniform), ("uniform box, sorted by x", ordered)):
        grid, b = build_leg(lines, name, pts, 0.8)
        ball_leg(lines, name, pts, grid, b, pts, 0.8, 16)
        knn_leg(lines, name, pts, grid, b, pts, 16)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
