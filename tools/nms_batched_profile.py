"""box2d_nms_batched (d3d_nms2d_grouped, k_nms_group) against the two ways a caller had before it, one process, HIP events:
  grouped   box2d_nms_batched on the whole batch (the stable sort of the ids, the segment offsets and the host read included);
  kernel    d3d_nms2d_grouped alone on prepared perm / seg_offsets (what a caller with fixed groups pays per call);
  (a) loop  box2d_nms on every group's rows, one call after the other (the row indices of the groups prepared outside the timed
            window, the gather of the rows inside it) -- code this operator does not touch;
  (b) offset one box2d_nms call on the batch with every group's boxes shifted apart (group number x 4096 in x): another
            rounding of every coordinate, so its mask may differ -- the number of differing rows is printed beside the time.
Workloads: 80 groups x 200 boxes, 80 x 500, 3000 x 8; rotated IoU, fp32 tensors, precise=True, detector-like clusters of 5-20
overlapping boxes per object.  Per workload the variants alternate inside every round (the same moments of the machine for
all of them); WARMUP rounds are dropped, then the median, minimum and maximum over the timed rounds, each variant between its own
pair of events per round.  The grouped mask is checked against the loop's, bit for bit, before anything is timed.
usage: python tools/nms_batched_profile.py [out.txt]   (writes profiles/nms_batched_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import _lib, synth                                                       # noqa: E402
from d3d_amd.box import IouType, box2d_nms, box2d_nms_batched                         # noqa: E402

WARMUP = 3
WORKLOADS = ((80, 200, 30), (80, 500, 30), (3000, 8, 7))          # (groups, boxes per group, timed rounds)
KW = dict(iou_method="rbox", iou_threshold=0.3, precise=True)
SHIFT = 4096.0


def clustered(n, seed):
    rng = np.random.default_rng(seed)
    objects, _ = synth.boxes2d_sparse(n // 5 + 1, seed + 1000)
    b = objects[np.repeat(np.arange(len(objects)), rng.integers(5, 21, len(objects)))[:n]].copy()
    b[:, :2] += rng.normal(0, 2.0, (n, 2))
    b[:, 2:4] *= rng.uniform(0.85, 1.15, (n, 2))
    b[:, 4] += rng.normal(0, 0.1, n)
    return b[rng.permutation(n)].astype(np.float32), rng.random(n).astype(np.float32)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nms_batched_profile.txt")
    assert torch.cuda.is_available(), "nms_batched_profile needs a GPU"
    torch.cuda.set_device(0)
    lib = _lib.load()
    lines = ["%s; rbox, fp32 tensors, precise=True, iou_threshold 0.3; %d warm-up rounds, then per variant the median [min .. max] "
             "of the timed rounds in ms, variants alternating inside a round, HIP events around each" % (torch.cuda.get_device_name(0), WARMUP),
             "%-12s %6s %-24s %-24s %-24s %-24s %9s %9s %s" % ("workload", "rounds", "grouped", "kernel", "(a) loop", "(b) offset",
                                                               "(a)/grp", "(b)/grp", "rows where (b) differs")]
    print("\n".join(lines), flush=True)
    for ngroups, per, rounds in WORKLOADS:
        n = ngroups * per
        rng = np.random.default_rng(ngroups)
        parts = [clustered(per, 17 * k + per) for k in range(ngroups)]
        ids = np.repeat(rng.choice(1 << 40, ngroups, replace=False), per)
        o = rng.permutation(n)
        b = torch.from_numpy(np.concatenate([p[0] for p in parts])[o]).cuda()
        s = torch.from_numpy(np.concatenate([p[1] for p in parts])[o]).cuda()
        g = torch.from_numpy(ids[o]).cuda()
        # prepared once: the groups' rows (loop), the shifted boxes (offset), perm / offsets (kernel)
        order, perm = torch.sort(g, stable=True)
        uniq, inverse, counts = torch.unique_consecutive(order, return_inverse=True, return_counts=True)
        seg = torch.zeros((ngroups + 1,), dtype=torch.int64, device="cuda")
        seg[1:] = counts.cumsum(0)
        rows = [perm[i * per:(i + 1) * per] for i in range(ngroups)]
        number = torch.empty_like(g)
        number[perm] = inverse
        shifted = b.clone()
        shifted[:, 0] += number.to(torch.float32) * SHIFT
        keep_raw = torch.empty((n,), dtype=torch.uint8, device="cuda")
        ws = torch.empty((max(lib.d3d_nms2d_grouped_workspace_bytes(n, ngroups), 1),), dtype=torch.uint8, device="cuda")

        def grouped():
            return box2d_nms_batched(b, s, g, **KW)

        def kernel():
            _lib.check(lib.d3d_nms2d_grouped(_lib.ptr(b), _lib.ptr(s), _lib.ptr(perm), _lib.ptr(seg), n, ngroups, per, int(IouType.RBOX),
                                             _lib.F32_WIDE, KW["iou_threshold"], 0.0, _lib.ptr(keep_raw), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr(), 0), "nms2d_grouped")
            return keep_raw

        def loop():
            keep = torch.empty((n,), dtype=torch.bool, device="cuda")
            for idx in rows:
                keep[idx] = box2d_nms(b[idx], s[idx], **KW)
            return keep

        def offset():
            return box2d_nms(shifted, s, **KW)

        exp = loop()
        assert torch.equal(grouped(), exp) and torch.equal(kernel().view(torch.bool), exp), "the grouped mask is not the loop's"
        differs = int((offset() != exp).sum())
        variants = (grouped, kernel, loop, offset)
        ms = {f: [] for f in variants}
        for r in range(WARMUP + rounds):
            for f in variants:
                t = event_ms(f)
                if r >= WARMUP:
                    ms[f].append(t)
        med = {f: float(np.median(ms[f])) for f in variants}
        cell = lambda f: "%.4f [%.4f .. %.4f]" % (med[f], min(ms[f]), max(ms[f]))    # noqa: E731
        lines.append("%-12s %6d %-24s %-24s %-24s %-24s %8.1fx %8.1fx %d of %d" % (
            "%d x %d" % (ngroups, per), rounds, cell(grouped), cell(kernel), cell(loop), cell(offset), med[loop] / med[grouped],
            med[offset] / med[grouped], differs, n))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
