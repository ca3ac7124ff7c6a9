"""DetectionEvaluator.calc_stats_batch (d3d_deteval_batched) against what a caller had before it, one process, one device:
  batch   calc_stats_batch on the whole split (host preparation, upload, the launches, the fetch and the stats' dicts included);
  loop    [calc_stats(gt_f, dt_f) for every frame] -- code the batched call does not touch, so it is the baseline.
Splits: F in {100, 1000, 4000} frames of 50 x 20 and of 200 x 50 boxes (detections x ground truths), cut from one
synth.boxes3d_eval set per split (20 / 50 consecutive ground truths and 50 of their 60 / all of their 200 noisy detections per frame,
shuffled; labels 1 .. 3 of which 1 and 2 are evaluated, a detection carrying its ground truth's label four times out of five;
distinct random scores); min_overlaps 0.5 / 0.25, the default 40 thresholds; both settings of reference_compat.
Both variants return host objects, so the clock is the host's (perf_counter after a device synchronisation); the variants
alternate inside every round, WARMUP rounds are dropped, then median [min .. max] of the timed rounds.  The batch result is
checked against the loop's (== on the dicts, NaN-aware) before anything is timed.
usage: python tools/deteval_batch_profile.py [out.txt]   (writes profiles/deteval_batch_profile.txt by default)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import synth                                                             # noqa: E402
from d3d_amd.benchmarks import DetectionEvaluator                                     # noqa: E402

WARMUP = 1
SPLITS = ((100, 7), (1000, 3), (4000, 2))              # (frames, timed rounds)
SHAPES = ((50, 20, 3), (200, 50, 4))                   # (detections, ground truths, detections drawn per ground truth)


def split(frames, n, m, rep, seed):
    rng = np.random.default_rng(seed)
    pred, gt = synth.boxes3d_eval(frames * m, rep, seed)
    gt9 = np.concatenate([rng.integers(1, 4, (len(gt), 1)), np.zeros((len(gt), 1)), gt], 1).astype(np.float32)
    label = np.where(rng.random(len(pred)) < 0.8, np.repeat(gt9[:, 0], rep), rng.integers(1, 4, len(pred)))
    score = (rng.permutation(len(pred)) + 0.5) / len(pred)
    dt9 = np.concatenate([label[:, None], score[:, None], pred], 1).astype(np.float32)
    rows = np.concatenate([f * m * rep + rng.permutation(m * rep)[:n] for f in range(frames)])
    return gt9, np.ascontiguousarray(dt9[rows]), np.arange(frames + 1, dtype=np.int64) * m, np.arange(frames + 1, dtype=np.int64) * n


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def clock_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "deteval_batch_profile.txt")
    assert torch.cuda.is_available(), "deteval_batch_profile needs a GPU"
    torch.cuda.set_device(0)
    lines = ["%s; classes [1, 2], min_overlaps [0.5, 0.25], 40 thresholds; %d warm-up round(s), then per variant the median [min .. max] of "
             "the timed rounds, ms per split on the host's clock, variants alternating inside a round" % (torch.cuda.get_device_name(0), WARMUP),
             "%-18s %-7s %6s %-30s %-30s %10s %10s %8s" % ("split", "compat", "rounds", "batch ms", "loop ms", "batch us/f", "loop us/f",
                                                         "loop/batch")]
    print("\n".join(lines), flush=True)
    for frames, rounds in SPLITS:
        for n, m, rep in SHAPES:
            gt, dt, go, do = split(frames, n, m, rep, 7 + frames + n)
            for compat in (True, False):
                ev = DetectionEvaluator([1, 2], [0.5, 0.25], reference_compat=compat)
                batch = lambda: ev.calc_stats_batch(gt, dt, go, do)
                loop = lambda: [ev.calc_stats(gt[go[f]:go[f + 1]], dt[do[f]:do[f + 1]]) for f in range(frames)]
                assert all(same(a, b) for a, b in zip(batch(), loop())), (frames, n, m, compat)
                tb, tl = [], []
                for r in range(WARMUP + rounds - 1):                # (the check above was a warm-up round of both already)
                    b, l = clock_ms(batch), clock_ms(loop)
                    if r >= WARMUP - 1:
                        tb.append(b)
                        tl.append(l)
                mb, ml = float(np.median(tb)), float(np.median(tl))
                fmt = lambda t, med: "%9.2f [%9.2f .. %9.2f]" % (med, min(t), max(t))
                lines.append("%-18s %-7s %6d %-30s %-30s %10.1f %10.1f %8.1f" % (
                    "%d x (%d x %d)" % (frames, n, m), compat, len(tb), fmt(tb, mb), fmt(tl, ml), mb * 1e3 / frames, ml * 1e3 / frames, ml / mb))
                print(lines[-1], flush=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
