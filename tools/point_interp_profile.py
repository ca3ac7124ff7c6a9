"""knn_query and point_interpolate (csrc/psample.hip, csrc/vinterp.hip) against what a user had without them: torch alone.

  kNN, fp32     (centres M x points N, k): 16384 x 4096 k 3 and 4096 x 1024 k 3 (the two upper feature-propagation layers of a KITTI
                PointNet++: every point of a level asks the FPS samples of the next), 16384 x 16384 k 16 (a DGCNN-style neighbourhood),
                100000 x 100000 k 3 (reported, not promised: the kernel is O(M N), a grid would do this one)
    torch       cdist [M, N] + topk(k, largest=False): the matrix the operator does not need, materialised (in slabs of centres once it
                passes 2^30 elements); it takes a square root and breaks ties its own way, so the share of equal ROWS is reported
  interpolate   the first shape, C = 128 and 256, fp32 and bf16: forward, and forward + backward
    torch       (feat[table] * weights[..., None]).sum(1) and its autograd: a [M, k, C] buffer forward, a float-atomic index_add_ backward
  Every figure measured is written down with the peak memory of the leg; a leg where the kernel is slower is marked LOSES.  The A/B
  of the kNN kernel's variants is a recorded block that this tool copies to the end of the file.

Timing: WARMUP untimed rounds, then ROUNDS timed ones (fewer for the slow legs), HIP events around each call, median [min .. max] in
ms.  Results are compared before anything is timed and the outcome is written next to the numbers.

usage: python tools/point_interp_profile.py [out.txt]   (writes profiles/point_interp_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                                   # noqa: E402
from d3d_amd.point import PointInterp, furthest_point_sample, knn_query, point_interpolate  # noqa: E402

WARMUP, ROUNDS, SLOW_ROUNDS = 2, 10, 3
SLAB = 2 ** 30                     # elements of the cdist matrix a torch leg holds at a time

# Recorded ONCE, with code that is no longer anywhere in the library: k_knn_query<float> ("library") against variants built from the same
# source in a stand-alone program (raw kernels, one segment, fp32, rows of 4 floats, median of 10 launches, tables compared with the
# library's).  "same walk, in this file" is the library's algorithm compiled there: it runs 0.90-0.98 x, the handicap every variant
# carries.  SEVERAL CENTRES PER WAVEFRONT (each loaded row judged against 2 or 4 centres, as many held sets): wins where the centres
# fill the chip many times over and insertions are rare (1.05-1.14 x at M 16384 and k <= 16, 1.28-1.55 x at 100 000 x 100 000), loses
# where they do not (0.57-0.81 x at M 4096: a quarter of the wavefronts) and wherever insertions dominate, which one wavefront then
# does for all its centres in turn (0.94-0.97 x at k 64, 0.46-0.70 x on rows sorted by descending distance).  Not kept: it would need a
# route per size and a fallback for wavefronts whose centres straddle two segments; a size-gated route is a possible follow-up.
# BITONIC MERGE of a tile whose ballot has more than 16 / 32 bits (the first tile is such a tile: this is also the bitonic seed): wins
# only where insertions dominate (1.05 x at k 64, 2.2-2.6 x on descending rows) and loses 0.82-0.95 x on every shape of the profile
# (58 cross-lane exchanges of a 64-bit key against the handful of insertions an unordered tile needs).  Not kept.
VARIANT_AB = """
A/B of the kNN kernel's variants, recorded once (neither was kept: several centres per wavefront wins only where M fills the chip many times over and loses at M 4096 and where insertions dominate; the bitonic merge / seed wins only where insertions dominate and loses on every shape above):
M  16384 x N   4096 k  3 unordered rows  library k_knn_query    0.0602 ms (1115.5 G pairs/s)
    same walk, in this file         0.0657 ms  library/variant  0.92x  same table True
    2 centres per wavefront         0.0575 ms  library/variant  1.05x  same table True
    4 centres per wavefront         0.0540 ms  library/variant  1.11x  same table True
    bitonic merge above 16 bits     0.0695 ms  library/variant  0.87x  same table True
    bitonic merge above 32 bits     0.0692 ms  library/variant  0.87x  same table True
M   4096 x N   1024 k  3 unordered rows  library k_knn_query    0.0120 ms ( 349.5 G pairs/s)
    same walk, in this file         0.0122 ms  library/variant  0.98x  same table True
    2 centres per wavefront         0.0148 ms  library/variant  0.81x  same table True
    4 centres per wavefront         0.0211 ms  library/variant  0.57x  same table True
    bitonic merge above 16 bits     0.0132 ms  library/variant  0.91x  same table True
    bitonic merge above 32 bits     0.0132 ms  library/variant  0.91x  same table True
M  16384 x N  16384 k 16 unordered rows  library k_knn_query    0.2300 ms (1166.9 G pairs/s)
    same walk, in this file         0.2496 ms  library/variant  0.92x  same table True
    2 centres per wavefront         0.2148 ms  library/variant  1.07x  same table True
    4 centres per wavefront         0.2023 ms  library/variant  1.14x  same table True
    bitonic merge above 16 bits     0.2470 ms  library/variant  0.93x  same table True
    bitonic merge above 32 bits     0.2430 ms  library/variant  0.95x  same table True
M  16384 x N  16384 k 64 unordered rows  library k_knn_query    0.3808 ms ( 704.8 G pairs/s)
    same walk, in this file         0.4090 ms  library/variant  0.93x  same table True
    2 centres per wavefront         0.3943 ms  library/variant  0.97x  same table True
    4 centres per wavefront         0.4036 ms  library/variant  0.94x  same table True
    bitonic merge above 16 bits     0.3628 ms  library/variant  1.05x  same table True
    bitonic merge above 32 bits     0.3633 ms  library/variant  1.05x  same table True
M 100000 x N 100000 k  3 unordered rows  library k_knn_query    4.8709 ms (2053.0 G pairs/s)
    same walk, in this file         5.4033 ms  library/variant  0.90x  same table True
    2 centres per wavefront         3.8134 ms  library/variant  1.28x  same table True
    4 centres per wavefront         3.1385 ms  library/variant  1.55x  same table True
    bitonic merge above 16 bits     5.9495 ms  library/variant  0.82x  same table True
    bitonic merge above 32 bits     5.9287 ms  library/variant  0.82x  same table True
M   4096 x N  16384 k 16 rows by DESCENDING distance  library k_knn_query    1.8226 ms (  36.8 G pairs/s)
    same walk, in this file         1.8721 ms  library/variant  0.97x  same table True
    2 centres per wavefront         2.5888 ms  library/variant  0.70x  same table True
    4 centres per wavefront         4.0002 ms  library/variant  0.46x  same table True
    bitonic merge above 16 bits     0.7048 ms  library/variant  2.59x  same table True
    bitonic merge above 32 bits     0.8409 ms  library/variant  2.17x  same table True
"""


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, rounds):
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


def torch_knn(x, c, k):
    """-> (rows [M, k] int64, squared distances): cdist + topk, slab by slab"""
    x3, c3 = x[:, :3].contiguous(), c[:, :3].contiguous()
    step = max(1, SLAB // max(1, x3.shape[0]))
    idx, d2 = [], []
    for a in range(0, c3.shape[0], step):
        top = torch.cdist(c3[a:a + step], x3).topk(k, dim=1, largest=False)
        idx.append(top.indices)
        d2.append(top.values ** 2)
    return torch.cat(idx), torch.cat(d2)


def emit(lines, text):
    lines.append(text)
    print(text, flush=True)


def knn_leg(lines, name, pts, ctr, k, rounds):
    table, dist2 = knn_query(pts, ctr, k)
    want, _ = torch_knn(pts, ctr, k)
    same = float((table.long() == want).all(1).float().mean())
    sets = float((table.long().sort(1).values == want.sort(1).values).all(1).float().mean())
    t_ours, m_ours = timed(lambda: knn_query(pts, ctr, k), rounds)
    t_torch, m_torch = timed(lambda: torch_knn(pts, ctr, k), min(rounds, SLOW_ROUNDS))
    mo, mt = float(np.median(t_ours)), float(np.median(t_torch))
    pairs = pts.shape[0] * ctr.shape[0]
    emit(lines, "knn %-22s M %6d x N %6d k %2d  ours %s ms (%6.1f G pairs/s, peak %s)   cdist + topk %s ms (peak %s)   torch/ours %6.1fx%s   rows equal "
         "to torch's: %.4f (as sets: %.4f)" % (name, ctr.shape[0], pts.shape[0], k, cell(t_ours), pairs / mo / 1e6, mib(m_ours), cell(t_torch), mib(m_torch),
                                             mt / mo, "" if mo < mt else "  LOSES", same, sets))


def torch_interp(feat, table, weights):
    return (feat[table] * weights[..., None].to(feat.dtype)).sum(1)


def interp_leg(lines, known, unknown, k, c, dtype):
    itp = PointInterp(known, unknown, k)
    itp.transpose()                                      # built once per frame and layer: not part of a call
    table = itp.table.long()
    gen = torch.Generator().manual_seed(c)
    feat = torch.randn((known.shape[0], c), generator=gen).to(dtype).cuda().requires_grad_()
    grad = torch.randn((unknown.shape[0], c), generator=gen).to(dtype).cuda()
    ours, theirs = point_interpolate(feat, itp), torch_interp(feat, table, itp.weights)
    err = float((ours.float() - theirs.float()).abs().max())
    g_ours, = torch.autograd.grad(ours, feat, grad)
    g_theirs, = torch.autograd.grad(theirs, feat, grad)
    gerr = float((g_ours.float() - g_theirs.float()).abs().max())

    def both(fn):
        def run():
            out = fn()
            torch.autograd.grad(out, feat, grad)
        return run

    def fwd_ours():
        return point_interpolate(feat, itp)

    def fwd_torch():
        return torch_interp(feat, table, itp.weights)

    for what, f_ours, f_torch in (("forward           ", fwd_ours, fwd_torch), ("forward + backward", both(fwd_ours), both(fwd_torch))):
        t_ours, m_ours = timed(f_ours, ROUNDS)
        t_torch, m_torch = timed(f_torch, ROUNDS)
        mo, mt = float(np.median(t_ours)), float(np.median(t_torch))
        emit(lines, "interpolate %s M %6d x N %6d k %d C %3d %-8s  ours %s ms (peak %s)   gather * w .sum %s ms (peak %s)   torch/ours %6.1fx%s   max "
             "|ours - torch| out %.3g grad %.3g" % (what, unknown.shape[0], known.shape[0], k, c, str(dtype).replace("torch.", ""), cell(t_ours), mib(m_ours),
                                                   cell(t_torch), mib(m_torch), mt / mo, "" if mo < mt else "  LOSES", err, gerr))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "point_interp_profile.txt")
    assert torch.cuda.is_available(), "point_interp_profile needs a GPU"
    torch.cuda.set_device(0)
    lines = []
    emit(lines, "%s; %d warm-up rounds, then the median [min .. max] of %d timed rounds (%d for the slow legs) in ms, HIP events around each call; "
         "peak = bytes allocated above the leg's inputs while it was timed" % (torch.cuda.get_device_name(0), WARMUP, ROUNDS, SLOW_ROUNDS))
    emit(lines, "kNN: one wavefront per centre walks its segment, O(M N) by design; the torch leg builds the [M, N] matrix (in slabs of 2^30 elements)")
    cloud = torch.from_numpy(synth.lidar_like(16384, 3)).cuda()
    level1 = cloud[furthest_point_sample(cloud, 4096)].contiguous()
    level2 = level1[furthest_point_sample(level1, 1024)].contiguous()
    knn_leg(lines, "FP layer 16384 <- 4096", level1, cloud, 3, ROUNDS)
    knn_leg(lines, "FP layer 4096 <- 1024", level2, level1, 3, ROUNDS)
    knn_leg(lines, "neighbourhood k 16", cloud, cloud, 16, ROUNDS)
    big = torch.from_numpy(synth.lidar_like(100000, 4)).cuda()
    knn_leg(lines, "whole cloud (reported)", big, big, 3, SLOW_ROUNDS)
    for dtype in (torch.float32, torch.bfloat16):
        for c in (128, 256):
            interp_leg(lines, level1, cloud, 3, c, dtype)
    lines.extend(VARIANT_AB.strip("\n").splitlines())
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
