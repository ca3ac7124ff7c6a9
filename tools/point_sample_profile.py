"""furthest_point_sample and ball_query (csrc/psample.hip) against what a user had without them: torch alone.

  FPS, fp32   (N, M, B) = (16384, 2048, 1 / 4 / 16) and (4096, 1024, 8) on the register routes, (180000, 4096, 1) on the streaming
              route; ms per call and us per step (ms / M: the B segments run side by side, one workgroup each)
    torch     the loop a user writes: per step an argmax, a gather and a fused-by-hand distance update over [B, N], M dependent
              steps of several launches each.  It is LAUNCH-BOUND (a step is a handful of ~10 us launches whatever N is), so the ratio
              says more about launch overhead than about the kernel: it flatters us.
  ball query  M = 2048 keypoints per sample (FPS of the cloud) against N = 16384 and N = 150000, nsample 16 / 32, r = 1 m
    torch     cdist [M, N], rows inside keep their number and the others get N, sort, the first nsample columns: the matrix the
              operator does not need, materialised and sorted
  Every figure measured is written down; a leg where the kernel is slower is marked LOSES.  The A/B of the ball query against an
  LDS-tile variant (lost, removed) is a recorded block that this tool copies to the end of the file.

Timing: WARMUP untimed rounds, then ROUNDS timed ones (fewer for the slow torch legs), HIP events around each call, median [min ..
max] in ms.  Results are compared before anything is timed and the outcome is written next to the numbers.

usage: python tools/point_sample_profile.py [out.txt]   (writes profiles/point_sample_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                   # noqa: E402
from d3d_amd.point import ball_query, fps_plan, furthest_point_sample      # noqa: E402

WARMUP, ROUNDS, SLOW_ROUNDS = 2, 10, 3
ROUTES = {0: "registers", 1: "registers", 2: "registers", 3: "registers + LDS", 4: "streaming"}


# Recorded ONCE, with code that is no longer in the library: k_ball_query ("wave") against a variant in which the 16 centres of a
# workgroup of 1024 lanes shared tiles of 1024 rows through LDS ("tile": two barriers per tile, a workgroup-uniform exit), the raw
# entries, fp32, median of 15 calls, identical tables.  The variant lost on every leg (0.80-0.92 x) and was removed: the walk is bound
# by each wavefront's own chain (2048 and 4096 centres against 150 000 rows take the same time), not by L2 bandwidth, and the
# barriers tie the fast waves of a workgroup to the slowest.  Eight tiles in flight instead of four: 0.446 against 0.459 ms, not kept.
TILE_AB = """
A/B, recorded once (the LDS-tile variant lost and was removed; eight tiles in flight instead of four: 0.446 against 0.459 ms at N 150000, not kept):
N  16384 x B 1  M 2048  r 1.0 nsample 16  full balls   5.0 %  wave 0.0606 ms  tile 0.0705 ms  wave/tile 0.86x  same True
N  16384 x B 1  M 2048  r 1.0 nsample 32  full balls   1.8 %  wave 0.0610 ms  tile 0.0700 ms  wave/tile 0.87x  same True
N  16384 x B 1  M 2048  r 4.0 nsample 16  full balls  98.7 %  wave 0.0560 ms  tile 0.0648 ms  wave/tile 0.86x  same True
N  16384 x B 1  M 2048  r 4.0 nsample 32  full balls  88.4 %  wave 0.0583 ms  tile 0.0700 ms  wave/tile 0.83x  same True
N 150000 x B 1  M 2048  r 1.0 nsample 16  full balls  34.5 %  wave 0.4542 ms  tile 0.5146 ms  wave/tile 0.88x  same True
N 150000 x B 1  M 2048  r 1.0 nsample 32  full balls  17.6 %  wave 0.4492 ms  tile 0.5183 ms  wave/tile 0.87x  same True
N 150000 x B 1  M 2048  r 4.0 nsample 16  full balls 100.0 %  wave 0.0967 ms  tile 0.1072 ms  wave/tile 0.90x  same True
N 150000 x B 1  M 2048  r 4.0 nsample 32  full balls 100.0 %  wave 0.2314 ms  tile 0.2525 ms  wave/tile 0.92x  same True
N  16384 x B 1  M  256  r 1.0 nsample 16  full balls   3.9 %  wave 0.0589 ms  tile 0.0678 ms  wave/tile 0.87x  same True
N  16384 x B 1  M  256  r 1.0 nsample 32  full balls   0.8 %  wave 0.0606 ms  tile 0.0696 ms  wave/tile 0.87x  same True
N  16384 x B 1  M  256  r 4.0 nsample 16  full balls  95.7 %  wave 0.0569 ms  tile 0.0668 ms  wave/tile 0.85x  same True
N  16384 x B 1  M  256  r 4.0 nsample 32  full balls  81.2 %  wave 0.0579 ms  tile 0.0696 ms  wave/tile 0.83x  same True
N 150000 x B 1  M 4096  r 1.0 nsample 16  full balls  36.2 %  wave 0.4623 ms  tile 0.5159 ms  wave/tile 0.90x  same True
N 150000 x B 1  M 4096  r 1.0 nsample 32  full balls  18.7 %  wave 0.4395 ms  tile 0.5174 ms  wave/tile 0.85x  same True
N 150000 x B 1  M 4096  r 4.0 nsample 16  full balls 100.0 %  wave 0.0932 ms  tile 0.1062 ms  wave/tile 0.88x  same True
N 150000 x B 1  M 4096  r 4.0 nsample 32  full balls 100.0 %  wave 0.2319 ms  tile 0.2532 ms  wave/tile 0.92x  same True
N  16384 x B 4  M 2048  r 1.0 nsample 16  full balls   4.9 %  wave 0.0838 ms  tile 0.0973 ms  wave/tile 0.86x  same True
N  16384 x B 4  M 2048  r 1.0 nsample 32  full balls   1.8 %  wave 0.0816 ms  tile 0.0940 ms  wave/tile 0.87x  same True
N  16384 x B 4  M 2048  r 4.0 nsample 16  full balls  98.7 %  wave 0.0667 ms  tile 0.0784 ms  wave/tile 0.85x  same True
N  16384 x B 4  M 2048  r 4.0 nsample 32  full balls  87.2 %  wave 0.0709 ms  tile 0.0886 ms  wave/tile 0.80x  same True
"""


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, rounds):
    for _ in range(WARMUP):
        fn()
    return [event_ms(fn) for _ in range(rounds)]


def cell(x):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(x)), min(x), max(x))


def torch_fps(x, m):
    """x [B, N, 3] -> [B, m]: the torch-only loop, in the rule's operation order"""
    b, n, _ = x.shape
    d = torch.full((b, n), float("inf"), device=x.device)
    out = torch.empty((b, m), dtype=torch.int64, device=x.device)
    rows = torch.arange(b, device=x.device)
    for s in range(m):
        c = torch.argmax(d, 1)
        out[:, s] = c
        diff = x - x[rows, c][:, None]
        q = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        d = torch.minimum(d, q)
    return out


def torch_ball(x, c, r, nsample):
    n = x.shape[0]
    dist = torch.cdist(c[:, :3].contiguous(), x[:, :3].contiguous())
    key = torch.where(dist < r, torch.arange(n, device=x.device), n).sort(1).values[:, :nsample]
    return torch.where(key < n, key, -1).int()


def fps_leg(lines, n, m, b):
    pts = torch.from_numpy(np.concatenate([synth.lidar_like(n, seed) for seed in range(b)])).cuda()
    offs = [n * i for i in range(b + 1)]
    route, cap = fps_plan(n)
    ours = furthest_point_sample(pts, m, offs)
    x = pts[:, :3].reshape(b, n, 3).contiguous()
    same = torch.equal(ours.view(b, m) - torch.tensor(offs[:-1], device="cuda")[:, None], torch_fps(x, m))
    t_ours = timed(lambda: furthest_point_sample(pts, m, offs), ROUNDS if route < 4 else SLOW_ROUNDS)
    t_torch = timed(lambda: torch_fps(x, m), SLOW_ROUNDS)
    mo, mt = float(np.median(t_ours)), float(np.median(t_torch))
    text = "fps N %6d M %4d B %2d  route %d (%s, capacity %d)  ours %s ms = %7.3f us/step   torch loop %s ms = %7.3f us/step   torch/ours %6.1fx%s   same indices: %s" % (
        n, m, b, route, ROUTES[route], cap, cell(t_ours), 1e3 * mo / m, cell(t_torch), 1e3 * mt / m, mt / mo, "" if mo < mt else "  LOSES", same)
    lines.append(text)
    print(text, flush=True)


def ball_leg(lines, n, m, r):
    pts = torch.from_numpy(synth.lidar_like(n, 3)).cuda()
    ctr = pts[furthest_point_sample(pts, m)].contiguous()
    for nsample in (16, 32):
        table, counts = ball_query(pts, ctr, r, nsample)
        want = torch_ball(pts, ctr, r, nsample)
        same = float((table == want).all(1).float().mean())
        t_ours = timed(lambda: ball_query(pts, ctr, r, nsample), ROUNDS)
        t_torch = timed(lambda: torch_ball(pts, ctr, r, nsample), SLOW_ROUNDS)
        mo, mt = float(np.median(t_ours)), float(np.median(t_torch))
        text = "ball N %6d M %4d nsample %2d r %.1f  (mean count %5.1f, %4.1f %% of the balls full)  ours %s ms   cdist + sort %s ms   torch/ours %6.1fx%s   rows equal to torch's: %.4f" % (
            n, m, nsample, r, float(counts.float().mean()), 100 * float((counts == nsample).float().mean()), cell(t_ours), cell(t_torch), mt / mo,
            "" if mo < mt else "  LOSES", same)
        lines.append(text)
        print(text, flush=True)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "point_sample_profile.txt")
    assert torch.cuda.is_available(), "point_sample_profile needs a GPU"
    torch.cuda.set_device(0)
    lines = ["%s; %d warm-up rounds, then the median [min .. max] of %d timed rounds (%d for the torch legs and the streaming route) in ms, HIP "
             "events around each call" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS, SLOW_ROUNDS),
             "the torch FPS loop is launch-bound (several launches per step, M dependent steps): its ratio flatters the kernel",
             "ball query: one wavefront per centre reads its tiles from L2; the A/B against a variant that shares the point tile of a "
             "workgroup's centres through LDS stands at the end of this file (recorded once; the variant lost and was removed)"]
    print("\n".join(lines), flush=True)
    for n, m, b in ((16384, 2048, 1), (16384, 2048, 4), (16384, 2048, 16), (4096, 1024, 8), (180000, 4096, 1)):
        fps_leg(lines, n, m, b)
    for n in (16384, 150000):
        ball_leg(lines, n, 2048, 1.0)
    lines.extend(TILE_AB.strip("\n").splitlines())
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
