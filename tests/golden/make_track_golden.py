"""Generate tests/golden/track_ref_cases.npz by running the REAL reference DetectionEvaluator / TrackingEvaluator
(d3d/benchmarks.pyx:1-890) with the REAL ScoreMatcher.match / BaseMatcher.match_by_order (d3d/tracking/matcher.pyx) in this
container.  Data only: the reference's text is read at run time, compiled in a temporary directory and thrown away.

What is taken as it is:
  * benchmarks.pyx from `bisect` (:23) up to SegmentationStats (:891): calc_precision / calc_recall / calc_fscore, quatdiff,
    DetectionEvalStats, DetectionEvaluator, TrackingEvalStats, TrackingEvaluator;
  * d3d/math/__init__.pxd: wmean, diffnorm3, cross3;
  * matcher.pyx: BaseMatcher.clear_match, match, match_by_order, query_src_match, query_dst_match, num_of_matches and
    ScoreMatcher.match.
Edits, all mechanical:
  * the module header: the cimports of :1-21 are replaced by the libc / libcpp ones they resolve to; NAN, isnan, isinf,
    INFINITY come from libc.math and PI is libc's M_PI (numpy.math is gone from numpy 2); the `addict` import is dropped
    (unused by these classes);
  * the classes of d3d.abstraction, which need the un-vendored dgal, are minimal stand-ins written here: ObjectTag (labels,
    scores), ObjectTarget3D (position_, dimension_, orientation_ as the yaw quaternion (0, 0, sin(yaw/2), cos(yaw/2)),
    orientation_var = 0, tid, tag), Target3DArray (a list with frame, get, size, to_numpy in the [n,9] layout), TransformSet
    (empty: every case is in one frame); DistanceTypes is the enum of matcher.pxd;
  * BaseMatcher.prepare_boxes (which needs dgal) is a stand-in that takes its distance cache from oracle.prepare_boxes (the
    same 1 - box3dr_iou after the +-1e3 clip, matcher.pyx:46-80);
  * matcher.pxd's class declarations (attributes, ScoreMatcher(BaseMatcher)) are restated in front of the bodies.
Nothing could not be compiled.

Cases: seeded sequences of tracking_sequence (moving boxes, dropouts, id swaps, false tracks), a sequence with classes outside
`classes`, and small hand-made sequences (empty frames, tracks that vanish and return).  They avoid the reference's undefined
cases: tids are unique per frame and > 0 for every selected detection, scores are distinct, every class has ground truths,
and no carried ground truth is of a class outside `classes`.  Recorded: per-frame TrackingEvalStats and DetectionEvalStats, the accumulated
metrics of both evaluators (ap, summary included) as JSON, and the reference's single-core time per frame.

usage: python tests/golden/make_track_golden.py [path/to/d3d]"""
import importlib
import json
import math
import os
import subprocess
import sys
import tempfile
import time
from enum import Enum

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

HEADER = """# cython: language_level=3, boundscheck=False, wraparound=False, cdivision=True
# distutils: language = c++
# distutils: include_dirs = %s
cimport cython
from cython.operator cimport dereference as deref
import numpy as np
cimport numpy as np
import scipy.stats as sps
from enum import Enum, IntEnum
from libc.math cimport NAN, isnan, isinf, INFINITY, M_PI as PI, atan2, sqrt, fabs
from libc.stdint cimport uint8_t, uint16_t, uint32_t, uint64_t
from libcpp.vector cimport vector
from libcpp.unordered_map cimport unordered_map
from libcpp.unordered_set cimport unordered_set
from libcpp.pair cimport pair
import oracle

# ---- stand-ins for d3d.abstraction (written for this generator) ----
cdef class ObjectTag:
    cdef public object mapping
    cdef public vector[int] labels
    cdef public vector[float] scores
    def __init__(self, label, score):
        self.labels.push_back(label)
        self.scores.push_back(score)

cdef class ObjectTarget3D:
    cdef float[:] position_, dimension_
    cdef float[:] orientation_
    cdef public float orientation_var
    cdef public unsigned long long tid
    cdef public ObjectTag tag
    cdef public object row
    def __init__(self, row, tid):
        row = np.asarray(row, np.float32)
        self.row = row
        self.position_ = row[2:5].copy()
        self.dimension_ = row[5:8].copy()
        self.orientation_ = np.array([0, 0, np.sin(row[8] / 2), np.cos(row[8] / 2)], np.float32)
        self.orientation_var = 0
        self.tid = tid
        self.tag = ObjectTag(int(row[0]), float(row[1]))

cdef class Target3DArray(list):
    cdef public str frame
    def __init__(self, rows, tids, frame="f"):
        list.__init__(self, [ObjectTarget3D(r, int(t)) for r, t in zip(rows, tids)])
        self.frame = frame
    cdef ObjectTarget3D get(self, int index):
        return <ObjectTarget3D>(list.__getitem__(self, index))
    cdef Py_ssize_t size(self):
        return len(self)
    def to_numpy(self):
        return np.asarray([o.row for o in self], np.float32).reshape(-1, 9)

cdef class TransformSet:
    pass

class DistanceTypes(IntEnum):
    IoU = 1
    RIoU = 2
    Position = 3

"""

MATH_SEP = "\n# ---- d3d/math/__init__.pxd ----\n"

MATCHER_HEAD = """
# ---- matcher.pxd declarations + matcher.pyx bodies ----
cdef class BaseMatcher:
    cdef Target3DArray _src_boxes, _dst_boxes
    cdef float[:, :] _distance_cache
    cdef unordered_map[int, int] _src_assignment, _dst_assignment

    cpdef void prepare_boxes(self, Target3DArray src_boxes, Target3DArray dst_boxes, int distance_metric) except*:
        # stand-in: the cache of the CPU oracle (1 - box3dr_iou after the +-1e3 clip)
        self.clear_match()
        self._src_boxes = src_boxes
        self._dst_boxes = dst_boxes
        self._distance_cache = np.ascontiguousarray(oracle.prepare_boxes(src_boxes.to_numpy(), dst_boxes.to_numpy()), np.float32)

"""


def _between(src, start, end):
    i = src.index(start)
    j = src.index(end, i)
    return src[i:j]


def build_reference(d3d, tmp):
    bench = open(os.path.join(d3d, "benchmarks.pyx")).read()
    matcher = open(os.path.join(d3d, "tracking", "matcher.pyx")).read()
    math_pxd = open(os.path.join(d3d, "math", "__init__.pxd")).read()
    math_body = "\n".join(l for l in math_pxd.splitlines() if not l.startswith(("cimport cython", "from libc.math")))
    base = _between(matcher, "    cpdef void clear_match(self):", "    @cython.boundscheck(False)") + \
        _between(matcher, "    cpdef void match(self, vector[int] src_subset", "cdef class ScoreMatcher:")
    score = "cdef class ScoreMatcher(BaseMatcher):\n" + \
        _between(matcher, "cdef class ScoreMatcher:", "cdef class NearestNeighborMatcher:").split("\n", 1)[1]
    body = _between(bench, "cdef inline int bisect", "@cython.auto_pickle(True)\ncdef class SegmentationStats")
    src = HEADER % np.get_include() + MATH_SEP + math_body + MATCHER_HEAD + base + "\n" + score + "\n# ---- benchmarks.pyx ----\n" + body
    with open(os.path.join(tmp, "trackref.pyx"), "w") as f:
        f.write(src)
    subprocess.check_call([sys.executable, "-m", "Cython.Build.Cythonize", "-i", "-q", "trackref.pyx"], cwd=tmp,
                          stdout=subprocess.DEVNULL)
    sys.path.insert(0, tmp)
    return importlib.import_module("trackref")


class Cls(Enum):
    Car = 1
    Pedestrian = 2
    Cyclist = 3


def _box(cls, x, score, y=0.0):
    return [cls, score, x, y, 0.0, 4.0, 2.0, 1.5, 0.0]


def hand_sequences():
    """empty frames on either side; a track that vanishes and returns; a detection drifting away from its ground truth"""
    f = []
    f.append(([_box(1, 0, 1), _box(2, 10, 1)], [_box(1, 0.1, .9), _box(2, 10.1, .8)], [1, 2], [11, 12]))
    f.append(([], [_box(1, 0.1, .9)], [], [11]))
    f.append(([_box(1, 0, 1), _box(2, 10, 1)], [], [1, 2], []))
    f.append(([_box(1, 0, 1), _box(2, 10, 1)], [_box(2, 10.1, .8)], [1, 2], [12]))
    f.append(([_box(1, 0, 1), _box(2, 10, 1)], [_box(1, 0.1, .9), _box(2, 10.1, .8)], [1, 2], [11, 12]))
    f.append(([_box(1, 0, 1), _box(2, 10, 1)], [_box(1, 1.4, .9), _box(1, 0.2, .7), _box(2, 10.1, .8)], [1, 2], [11, 13, 12]))
    f.append(([_box(1, 0, 1), _box(2, 10, 1)], [_box(1, 0.1, .6), _box(1, 0.3, .95), _box(2, 10.1, .8)], [2, 1], [11, 13, 12]))
    gt = [np.asarray(x[0], np.float32).reshape(-1, 9) for x in f]
    dt = [np.asarray(x[1], np.float32).reshape(-1, 9) for x in f]
    gi = [np.asarray(x[2], np.uint64) for x in f]
    di = [np.asarray(x[3], np.uint64) for x in f]
    return gt, dt, gi, di


def split(seq):
    g, d, gi, di, go, do = seq
    F = len(go) - 1
    return ([g[go[k]:go[k + 1]] for k in range(F)], [d[do[k]:do[k + 1]] for k in range(F)],
            [gi[go[k]:go[k + 1]] for k in range(F)], [di[do[k]:do[k + 1]] for k in range(F)])


def jsonable(x):
    if isinstance(x, dict):
        return {str(k.value if isinstance(k, Enum) else k): jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    if isinstance(x, (np.floating, float)):
        return float(x)
    if isinstance(x, (np.integer, int)):
        return int(x)
    return x


def metrics(ev, tracking):
    """every metric method of the accumulated evaluator, as JSON-able data"""
    out = dict(gt_count=ev.gt_count(), ap=ev.ap(), summary=ev.summary(), summary_verbose=ev.summary(verbose=True),
               fscore_all=ev.fscore(return_all=True), precision_all=ev.precision(return_all=True),
               recall_all=ev.recall(return_all=True))
    for s in (float("nan"), 0.0, 0.35, 0.8):
        key = "nan" if math.isnan(s) else "%g" % s
        for name in ("dt_count", "tp", "fp", "fn", "precision", "recall", "fscore", "acc_iou", "acc_box", "acc_dist", "acc_angular"):
            out["%s@%s" % (name, key)] = getattr(ev, name)(s)
        if tracking:
            for name in ("id_switches", "fragments", "mota", "tracked_ratio", "lost_ratio"):
                out["%s@%s" % (name, key)] = getattr(ev, name)(s)
    if tracking:
        out.update(gt_traj_count=ev.gt_traj_count(), tracked_ratio_all=ev.tracked_ratio(return_all=True),
                   lost_ratio_all=ev.lost_ratio(0.5, 0.3, return_all=True),
                   summary_note=ev.summary(0.5, 0.7, 0.3, note="golden", verbose=True))
    return json.dumps(jsonable(out))


def stats_arrays(st, classes, T, tracking):
    """a DetectionEvalStats / TrackingEvalStats as arrays [C, T] (class order = `classes`) and (class, t, tid, count) rows"""
    out = {"ngt": np.array([st.ngt[c] for c in classes], np.int64)}
    names = ["ndt", "tp", "fp", "fn"] + (["id_switches", "fragments"] if tracking else [])
    for k in names:
        out[k] = np.array([list(getattr(st, k)[c]) for c in classes], np.int64).reshape(len(classes), T)
    for k in ("acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var"):
        out[k] = np.array([list(getattr(st, k)[c]) for c in classes], np.float32).reshape(len(classes), T)
    if tracking:
        rows = [(c, 0, tid, n) for c in classes for tid, n in st.ngt_ids[c].items()]          # (t column unused)
        out["ngt_ids"] = np.array(rows, np.uint64).reshape(-1, 4)
        for k in ("ngt_tracked", "ndt_ids"):
            rows = [(c, t, tid, n) for c in classes for t in range(T) for tid, n in getattr(st, k)[c][t].items()]
            out[k] = np.array(rows, np.uint64).reshape(-1, 4)
    return out


def main():
    d3d = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/d3d"
    from d3d_amd import synth
    cases = [  # name, classes, min_overlaps, pr_sample_count, pr_sample_scale, frames
        ("seq_a", [Cls.Car, Cls.Pedestrian], 0.5, 40, "log10", split(synth.tracking_sequence(frames=10, n_tracks=20, seed=11))),
        ("seq_b", [Cls.Car, Cls.Pedestrian], [0.3, 0.6], 12, "lin", split(synth.tracking_sequence(frames=8, n_tracks=30, seed=12, swap=0.2))),
        ("seq_c", [Cls.Pedestrian], 0.5, 16, "log10", split(synth.tracking_sequence(frames=8, n_tracks=25, seed=13, dropout=0.3))),
        ("hand", [Cls.Car, Cls.Pedestrian], 0.5, 8, "lin", hand_sequences()),
    ]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ref = build_reference(d3d, tmp)
        for name, classes, overlaps, T, scale, (gts, dts, gis, dis) in cases:
            tev = ref.TrackingEvaluator(classes, overlaps, pr_sample_count=T, pr_sample_scale=scale)
            dev = ref.DetectionEvaluator(classes, overlaps, pr_sample_count=T, pr_sample_scale=scale)
            vals = [c.value for c in classes]
            p = name + "/"
            out[p + "classes"] = np.array(vals, np.int64)
            out[p + "params"] = np.array(json.dumps(dict(min_overlaps=overlaps, T=T, scale=scale)))
            out[p + "frames"] = np.array(len(gts))
            t_track = t_det = 0.0
            for f, (g, d, gi, di) in enumerate(zip(gts, dts, gis, dis)):
                G, D = ref.Target3DArray(g, gi), ref.Target3DArray(d, di)
                t0 = time.perf_counter()
                ts = tev.calc_stats(G, D)
                t1 = time.perf_counter()
                ds = dev.calc_stats(G, D)
                t2 = time.perf_counter()
                t_track, t_det = t_track + t1 - t0, t_det + t2 - t1
                tev.add_stats(ts)
                dev.add_stats(ds)
                q = p + "f%d/" % f
                out[q + "gt"], out[q + "dt"], out[q + "gt_tids"], out[q + "dt_tids"] = g, d, gi, di
                for k, v in stats_arrays(ts, vals, T, True).items():
                    out[q + "track/" + k] = v
                for k, v in stats_arrays(ds, vals, T, False).items():
                    out[q + "det/" + k] = v
            out[p + "track_metrics"] = np.array(metrics(tev, True))
            out[p + "det_metrics"] = np.array(metrics(dev, False))
            out[p + "time_per_frame_s"] = np.array([t_track / len(gts), t_det / len(gts)])
            print("%s: %d frames, reference %.2f ms / frame (tracking), %.2f ms (detection)" % (
                name, len(gts), 1e3 * t_track / len(gts), 1e3 * t_det / len(gts)))
        # the reference's single-core time on the profile's shape (tools/track_profile.py): ~100 gt x 150 dt
        g, d, gi, di, go, do = synth.tracking_sequence(frames=5, n_tracks=110, seed=1, false_tracks=50)
        tev = ref.TrackingEvaluator([Cls.Car, Cls.Pedestrian], 0.5)
        best = np.inf
        for f in range(5):
            G, D = ref.Target3DArray(g[go[f]:go[f + 1]], gi[go[f]:go[f + 1]]), ref.Target3DArray(d[do[f]:do[f + 1]], di[do[f]:do[f + 1]])
            t0 = time.perf_counter()
            tev.calc_stats(G, D)
            best = min(best, time.perf_counter() - t0)
        out["time/frame_100x150_s"] = np.array([best])
        print("100 x 150 frame: %.2f ms" % (best * 1e3))
    np.savez_compressed(os.path.join(HERE, "track_ref_cases.npz"), **out)
    print("wrote", len(cases), "cases")


if __name__ == "__main__":
    main()
