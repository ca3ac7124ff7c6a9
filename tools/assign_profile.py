"""HungarianMatcher / NearestNeighborMatcher / linear_sum_assignment on the GPU (d3d_lsap_batched, d3d_nn_match): wall time per
call (host preparation, launches and the fetch of the result included) of
  * a tracker-sized frame: 3 classes of 500, 250 and 100 boxes, Position distances (hungarian_match / nearest_neighbor_match);
  * 200 such frames queued one after the other (hungarian_match, one status read per frame);
  * a 2 k x 5 k frame (one class; linear_sum_assignment on the device matrix and hungarian_match);
per-kernel times from the library's event profiler; beside them scipy.optimize.linear_sum_assignment on one host core where
scipy is installed.  The reference's own single-core time on the tracker frame is recorded by
tests/golden/make_matcher_golden.py (time/*_tracker_frame_s in tests/golden/matcher_ref_cases.npz).
usage: python tools/assign_profile.py [out.json]   (writes profiles/assign_profile.{json,txt} by default)"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from d3d_amd import _lib                                                              # noqa: E402
from d3d_amd.tracking import hungarian_match, linear_sum_assignment, nearest_neighbor_match      # noqa: E402


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


def tracker_frame(seed, counts=(500, 250, 100)):
    rng = np.random.default_rng(seed)
    ps, pd, ls, ld = [], [], [], []
    for cls, k in enumerate(counts, 1):
        p = rng.uniform(-60, 60, (k, 3)).astype(np.float32)
        q = p + rng.normal(0, 1.0, p.shape).astype(np.float32)
        pd.append(p)
        ps.append(q[rng.permutation(k)])
        ls += [cls] * k
        ld += [cls] * k
    s, d = np.concatenate(ps), np.concatenate(pd)
    dist = np.sqrt(((s[:, None, :].astype(np.float64) - d[None]) ** 2).sum(-1)).astype(np.float32)
    return np.array(ls), np.array(ld), dist


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "assign_profile.json")
    torch.cuda.set_device(0)
    thr = {1: 2.0, 2: 1.0, 3: 3.0}
    ls, ld, dist = tracker_frame(1)
    d = torch.from_numpy(dist).cuda()
    frames = [tracker_frame(10 + k) for k in range(200)]
    dfr = [torch.from_numpy(f[2]).cuda() for f in frames]
    rng = np.random.default_rng(2)
    big = rng.random((2000, 5000)).astype(np.float32)
    dbig = torch.from_numpy(big).cuda()
    res = dict(frame_classes=[500, 250, 100], big_shape=[2000, 5000])
    res["hungarian_frame_ms"] = wall(lambda: hungarian_match(d, ls, ld, thr), 20)
    res["nn_frame_ms"] = wall(lambda: nearest_neighbor_match(d, ls, ld, thr), 20)
    res["hungarian_200_frames_ms"] = wall(lambda: [hungarian_match(dfr[k], frames[k][0], frames[k][1], thr) for k in range(200)], 2)
    res["lsap_big_ms"] = wall(lambda: linear_sum_assignment(dbig), 2)
    res["nn_big_ms"] = wall(lambda: nearest_neighbor_match(dbig, np.zeros(2000), np.zeros(5000), {0: 2.0}), 3)
    res["kernels_hungarian_frame"] = kernels(lambda: hungarian_match(d, ls, ld, thr))
    res["kernels_nn_frame"] = kernels(lambda: nearest_neighbor_match(d, ls, ld, thr))
    res["kernels_lsap_big"] = kernels(lambda: linear_sum_assignment(dbig))
    try:
        from scipy.optimize import linear_sum_assignment as sp_lsa
        def per_class(ls_, ld_, dd):
            for c in np.unique(ls_):
                sp_lsa(dd[np.ix_(np.nonzero(ls_ == c)[0], np.nonzero(ld_ == c)[0])])
        t0 = time.perf_counter()
        per_class(ls, ld, dist)
        res["scipy_frame_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for f in frames:
            per_class(*f)
        res["scipy_200_frames_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        sp_lsa(big)
        res["scipy_big_ms"] = (time.perf_counter() - t0) * 1e3
        # the same bits: the GPU's assignment equals scipy's
        a, b = linear_sum_assignment(big)
        ea, eb = sp_lsa(big)
        res["big_equals_scipy"] = bool(np.array_equal(a, ea) and np.array_equal(b, eb))
    except ImportError:
        res["scipy"] = "not installed"
    res["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    txt = os.path.splitext(out)[0] + ".txt"
    with open(txt, "w") as f:
        for k, v in res.items():
            f.write("%s: %s\n" % (k, v) if not isinstance(v, str) or "\n" not in v else "%s:\n%s\n" % (k, v))
    print(json.dumps({k: v for k, v in res.items() if not k.startswith("kernels")}))


if __name__ == "__main__":
    main()
