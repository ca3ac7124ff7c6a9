"""box2d_iou_paired / box3d_iou_paired (boxpair.hip) against the only route a caller had before them, one process, HIP events:
  (a) matrix  box2d_iou(b1, b2, method).diagonal() -- the [N,N] matrix for its N diagonal entries; with backward: the gradients of
              (diagonal * w).sum(), whose incoming gradient is zero off the diagonal.  iou3d has no gradient: forward only.
  (b) paired  the paired operator; with backward: the gradients of (values * w).sum().
Workloads: N = 512, 4096, 65536 matched pairs -- targets like a frame's boxes, predictions = targets moved, resized and turned a
little (a detector's regression pairs: almost all of them overlap); 'rbox' and 'grbox' in fp64, 3D 'rbox' in fp32.  At 65536
route (a) is not run: its matrix alone is N * N * 8 bytes (the line says how many).  Per workload the variants alternate inside
every round (the same moments of the machine for all of them); WARMUP rounds are dropped, then the median, minimum and maximum
over the timed rounds, each variant between its own pair of events per round.  The paired values are checked against the
matrix's diagonal, bit for bit, before anything is timed.
usage: python tools/paired_profile.py [out.txt]   (writes profiles/paired_profile.txt by default)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                             # noqa: E402
from d3d_amd.box import box2d_iou, box2d_iou_paired, box3d_iou_paired, iou3d          # noqa: E402

WARMUP = 3
SIZES = ((512, 30), (4096, 20), (65536, 30))                      # (pairs, timed rounds)
MATRIX_MAX = 4096
WORKLOADS = (("rbox", 2, np.float64), ("grbox", 2, np.float64), ("rbox", 3, np.float32))


def matched_pairs(n, dims, dtype, seed):
    rng = np.random.default_rng(seed)
    tgt, _ = synth.boxes2d_sparse(n, seed + 1000)
    pred = tgt.copy()
    pred[:, :2] += rng.normal(0, 0.3, (n, 2))
    pred[:, 2:4] *= rng.uniform(0.8, 1.25, (n, 2))
    pred[:, 4] += rng.normal(0, 0.1, n)
    if dims == 3:
        z, lz = rng.normal(0, 0.5, n), rng.uniform(1.2, 2.5, n)
        tgt = np.stack([tgt[:, 0], tgt[:, 1], z, tgt[:, 2], tgt[:, 3], lz, tgt[:, 4]], 1)
        pred = np.stack([pred[:, 0], pred[:, 1], z + rng.normal(0, 0.1, n), pred[:, 2], pred[:, 3], lz * rng.uniform(0.8, 1.25, n), pred[:, 4]], 1)
    return (torch.from_numpy(pred.astype(dtype)).cuda(), torch.from_numpy(tgt.astype(dtype)).cuda(),
            torch.from_numpy(rng.random(n).astype(dtype)).cuda())


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "paired_profile.txt")
    assert torch.cuda.is_available(), "paired_profile needs a GPU"
    torch.cuda.set_device(0)
    lines = ["%s; matched (prediction, target) pairs; %d warm-up rounds, then per variant the median [min .. max] of the timed rounds in ms, "
             "variants alternating inside a round, HIP events around each; fwd = values, f+b = values and both gradients"
             % (torch.cuda.get_device_name(0), WARMUP),
             "%-22s %6s %-26s %-26s %-26s %-26s %9s %9s" % ("workload", "rounds", "(a) matrix fwd", "(a) matrix f+b", "(b) paired fwd",
                                                            "(b) paired f+b", "fwd a/b", "f+b a/b")]
    print("\n".join(lines), flush=True)
    for n, rounds in SIZES:
        for method, dims, dtype in WORKLOADS:
            pred, tgt, w = matched_pairs(n, dims, dtype, n + dims)
            precise = dtype == np.float64
            paired_op = box2d_iou_paired if dims == 2 else box3d_iou_paired
            matrix_op = (lambda x, y: box2d_iou(x, y, method=method, precise=precise)) if dims == 2 else (lambda x, y: iou3d(x, y, method))

            def paired_fwd():
                return paired_op(pred, tgt, method=method, precise=precise)

            def paired_fb():
                p = pred.detach().requires_grad_(True)
                t = tgt.detach().requires_grad_(True)
                (paired_op(p, t, method=method, precise=precise) * w).sum().backward()
                return p.grad, t.grad

            def matrix_fwd():
                return matrix_op(pred, tgt).diagonal()

            def matrix_fb():
                p = pred.detach().requires_grad_(True)
                t = tgt.detach().requires_grad_(True)
                (matrix_op(p, t).diagonal() * w).sum().backward()
                return p.grad, t.grad

            variants = [paired_fwd, paired_fb]
            if n <= MATRIX_MAX:
                variants += [matrix_fwd] + ([matrix_fb] if dims == 2 else [])
                # (the matrix takes its multi-kernel routes at these sizes: the same per-pair functions, so the same bits)
                assert torch.equal(paired_fwd(), matrix_fwd()), "the paired values are not the matrix's diagonal"
                if dims == 2:
                    gp, gm = paired_fb(), matrix_fb()
                    scale = max(1.0, float(gm[0].abs().max()), float(gm[1].abs().max()))
                    assert max(float((gp[0] - gm[0]).abs().max()), float((gp[1] - gm[1]).abs().max())) < 1e-9 * scale, "gradients differ"
            ms = {f: [] for f in variants}
            for r in range(WARMUP + rounds):
                for f in variants:
                    t = event_ms(f)
                    if r >= WARMUP:
                        ms[f].append(t)
            med = {f: float(np.median(ms[f])) for f in variants}
            cell = lambda f: "%.4f [%.4f .. %.4f]" % (med[f], min(ms[f]), max(ms[f])) if f in ms else "-"      # noqa: E731
            ratio = lambda a, b: "%8.1fx" % (med[a] / med[b]) if a in ms else "%9s" % "-"                       # noqa: E731
            name = "%dD %s %s N=%d" % (dims, method, "fp64" if precise else "fp32", n)
            lines.append("%-22s %6d %-26s %-26s %-26s %-26s %s %s" % (name, rounds, cell(matrix_fwd), cell(matrix_fb), cell(paired_fwd),
                                                                       cell(paired_fb), ratio(matrix_fwd, paired_fwd), ratio(matrix_fb, paired_fb)))
            if n > MATRIX_MAX:
                lines[-1] += "   (a) infeasible: the [N,N] matrix alone is %d bytes (%.1f GB)" % (n * n * pred.element_size(), n * n * pred.element_size() / 1e9)
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
