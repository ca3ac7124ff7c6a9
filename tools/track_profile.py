"""TrackingEvaluator on the GPU (d3d_match_distance + d3d_track_frame): wall time per call of calc_stats on one ~100 gt x 150 dt
frame, of calc_stats_sequence on 200 such frames, and of calc_stats on one 2 k gt x 5 k dt frame (host preparation, launches
and the final fetch included); per-kernel times from the library's event profiler; beside them, the literal Python checker's
time per frame (tests/track_reference.py).  The reference's own single-core time for such a frame is recorded by
tests/golden/make_track_golden.py (time/frame_100x150_s in tests/golden/track_ref_cases.npz).
usage: python tools/track_profile.py [out.json]   (writes profiles/track_profile.{json,txt} by default)"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from d3d_amd import _lib, synth                         # noqa: E402
from d3d_amd.benchmarks import TrackingEvaluator        # noqa: E402


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def kernels(fn):
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.d3d_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    lib.d3d_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.d3d_profile_report(buf, len(buf))
    return buf.value.decode()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "track_profile.json")
    torch.cuda.set_device(0)
    seq = synth.tracking_sequence(frames=200, n_tracks=110, seed=1, false_tracks=50)
    g, d, gi, di, go, do = seq
    frame = (g[go[0]:go[1]], d[do[0]:do[1]], gi[go[0]:go[1]], di[do[0]:do[1]])
    big = synth.tracking_sequence(frames=1, n_tracks=2100, seed=2, false_tracks=3000)
    bigf = (big[0], big[1], big[2], big[3])
    ev = TrackingEvaluator([1, 2], 0.5)
    res = dict(frame_shape=[len(frame[0]), len(frame[1])], seq_frames=200, big_shape=[len(big[0]), len(big[1])])
    res["calc_stats_frame_ms"] = wall(lambda: ev.calc_stats(*frame), 50)
    res["calc_stats_sequence_200_ms"] = wall(lambda: ev.calc_stats_sequence(*seq), 5)
    res["calc_stats_big_frame_ms"] = wall(lambda: ev.calc_stats(*bigf), 5)
    res["kernels_frame"] = kernels(lambda: ev.calc_stats(*frame))
    res["kernels_sequence_200"] = kernels(lambda: ev.calc_stats_sequence(*seq))
    res["kernels_big_frame"] = kernels(lambda: ev.calc_stats(*bigf))
    t0 = time.perf_counter()
    ev.calc_stats_sequence(*seq)
    t1 = time.perf_counter()
    hs = [ev._prepare_host(g[go[f]:go[f + 1]], d[do[f]:do[f + 1]], gi[go[f]:go[f + 1]], di[do[f]:do[f + 1]]) for f in range(200)]
    t2 = time.perf_counter()
    res["host_prepare_200_ms"] = (t2 - t1) * 1e3
    res["sequence_once_ms"] = (t1 - t0) * 1e3
    try:
        import track_reference as tr
        from d3d_amd.tracking import DistanceTypes, prepare_boxes
        st = tr.State(40)
        md = {c: np.float32(v) for c, v in ev._max_distance.items()}
        cache = prepare_boxes(frame[1], frame[0], DistanceTypes.RIoU).cpu().numpy()
        t0 = time.perf_counter()
        tr.calc_stats(st, *frame, [1, 2], md, ev.score_thresholds, cache=cache)
        res["python_checker_frame_ms"] = (time.perf_counter() - t0) * 1e3
    except ImportError:
        pass
    del hs
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    lines = ["%s: %s" % (k, v) for k, v in res.items() if not k.startswith("kernels")]
    for k in ("kernels_frame", "kernels_sequence_200", "kernels_big_frame"):
        lines += ["", k + ":", res[k]]
    with open(os.path.splitext(out)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
