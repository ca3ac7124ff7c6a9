"""Generate tests/golden/matcher_ref_cases.npz by running the REAL reference BaseMatcher.match_by_order,
NearestNeighborMatcher.match and HungarianMatcher.match (d3d/tracking/matcher.pyx:84-230, which calls
scipy.optimize.linear_sum_assignment) in this container.  Data only: the reference's text is read at run time, compiled in a
temporary directory and thrown away.

What is taken as it is: matcher.pyx's BaseMatcher.clear_match, match, match_by_order, query_src_match, query_dst_match,
num_of_matches, NearestNeighborMatcher.match and HungarianMatcher.match, with scipy's linear_sum_assignment.
Edits, all mechanical:
  * the module header: the cimports of d3d.dgal / d3d.abstraction are replaced by minimal stand-ins written here -- ObjectTag
    (labels, scores), ObjectTarget3D (tag only), Target3DArray (a list with get); matcher.pxd's class declarations are restated
    in front of the bodies;
  * BaseMatcher.prepare_boxes (which needs dgal) is a stand-in that takes the distance cache as given (`set_cache`): every case
    records its fp32 matrix, so the cache's origin does not matter.
Nothing could not be compiled.

Cases (distances fp32): seeded frames of several classes (Position distances of moving boxes, 1 - rotated IoU from the CPU
oracle with many exact 1.0 entries), distances quantized to multiples of 0.25 (many ties), a constant matrix, rectangular
shapes both ways, unsorted subsets, a class without destinations, a tag missing from the threshold map, a distance exactly at
the threshold, and two `match` calls without clear_match.  Recorded after every call: the two assignment maps as arrays (-1 =
none), for both matchers.  NearestNeighborMatcher's order of equal distances is left open by the reference's unstable argsort:
a case records whether its subset matrix holds equal values (`nn_ties`); the tests compare the NN goldens only where it does
not.  Plus plain linear_sum_assignment results on tie-heavy matrices (1x1 .. 1000x3000; the large ones are regenerated from
their seed, with a checksum), and the reference's single-core time per frame on a tracker-sized frame.

usage: python tests/golden/make_matcher_golden.py [path/to/d3d]"""
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

HEADER = """# cython: language_level=3, boundscheck=False, wraparound=False, cdivision=True
# distutils: language = c++
# distutils: include_dirs = %s
cimport cython
import numpy as np
cimport numpy as np
from scipy.optimize import linear_sum_assignment
from libcpp.vector cimport vector
from libcpp.unordered_map cimport unordered_map

# ---- stand-ins for d3d.abstraction (written for this generator) ----
cdef class ObjectTag:
    cdef public vector[int] labels
    cdef public vector[float] scores
    def __init__(self, label, score):
        self.labels.push_back(label)
        self.scores.push_back(score)

cdef class ObjectTarget3D:
    cdef public ObjectTag tag
    def __init__(self, label):
        self.tag = ObjectTag(int(label), 0.0)

cdef class Target3DArray(list):
    def __init__(self, labels):
        list.__init__(self, [ObjectTarget3D(int(l)) for l in labels])
    cdef ObjectTarget3D get(self, int index):
        return <ObjectTarget3D>(list.__getitem__(self, index))

# ---- matcher.pxd declarations + matcher.pyx bodies ----
cdef class BaseMatcher:
    cdef Target3DArray _src_boxes, _dst_boxes
    cdef float[:, :] _distance_cache
    cdef unordered_map[int, int] _src_assignment, _dst_assignment

    def set_cache(self, src_labels, dst_labels, cache):
        # stand-in for prepare_boxes: the cache as given
        self.clear_match()
        self._src_boxes = Target3DArray(src_labels)
        self._dst_boxes = Target3DArray(dst_labels)
        self._distance_cache = np.ascontiguousarray(cache, np.float32)

"""


def _between(src, start, end=None):
    i = src.index(start)
    return src[i:src.index(end, i)] if end else src[i:]


def build_reference(d3d, tmp):
    matcher = open(os.path.join(d3d, "tracking", "matcher.pyx")).read()
    base = _between(matcher, "    cpdef void clear_match(self):", "    @cython.boundscheck(False)") + \
        _between(matcher, "    cpdef void match(self, vector[int] src_subset", "cdef class ScoreMatcher:")
    nn = "cdef class NearestNeighborMatcher(BaseMatcher):\n" + \
        _between(matcher, "cdef class NearestNeighborMatcher:", "cdef class HungarianMatcher:").split("\n", 1)[1]
    hu = "cdef class HungarianMatcher(BaseMatcher):\n" + _between(matcher, "cdef class HungarianMatcher:").split("\n", 1)[1]
    src = HEADER % np.get_include() + base + "\n" + nn + "\n" + hu
    with open(os.path.join(tmp, "matchref.pyx"), "w") as f:
        f.write(src)
    subprocess.check_call([sys.executable, "-m", "Cython.Build.Cythonize", "-i", "-q", "matchref.pyx"], cwd=tmp,
                          stdout=subprocess.DEVNULL)
    sys.path.insert(0, tmp)
    return importlib.import_module("matchref")


def position_frame(rng, counts, spread=40.0, jitter=1.5, extra=0.2):
    """src = dst moved a little, some dropped, some added; -> (labels_src, labels_dst, fp32 centre distances)"""
    ls, ld, ps, pd = [], [], [], []
    for cls, k in counts.items():
        p = rng.uniform(-spread, spread, (k, 3)).astype(np.float32)
        keep = rng.random(k) > extra
        q = p[keep] + rng.normal(0, jitter, (int(keep.sum()), 3)).astype(np.float32)
        add = rng.uniform(-spread, spread, (int(k * extra) + 1, 3)).astype(np.float32)
        q = np.concatenate([q, add])
        ps.append(q)
        pd.append(p)
        ls += [cls] * len(q)
        ld += [cls] * len(p)
    s, d = np.concatenate(ps), np.concatenate(pd)
    ps_, pd_ = rng.permutation(len(s)), rng.permutation(len(d))
    s, d = s[ps_], d[pd_]
    ls, ld = np.array(ls)[ps_], np.array(ld)[pd_]
    dist = np.sqrt(((s[:, None, :].astype(np.float64) - d[None, :, :]) ** 2).sum(-1)).astype(np.float32)
    return ls.astype(np.int64), ld.astype(np.int64), dist


def riou_frame(rng, n, m, classes=2):
    import oracle
    def boxes(k):
        b = np.zeros((k, 9), np.float32)
        b[:, 0] = rng.integers(0, classes, k)
        b[:, 2:4] = rng.uniform(-15, 15, (k, 2))
        b[:, 5:8] = rng.uniform(1, 4, (k, 3))
        b[:, 8] = rng.uniform(-3, 3, k)
        return b
    s, d = boxes(n), boxes(m)
    return s[:, 0].astype(np.int64), d[:, 0].astype(np.int64), np.ascontiguousarray(oracle.prepare_boxes(s, d), np.float32)


def cases(rng):
    out = []
    def case(name, ls, ld, dist, calls):
        out.append((name, np.asarray(ls, np.int64), np.asarray(ld, np.int64), np.asarray(dist, np.float32), calls))
    for k in range(3):
        ls, ld, d = position_frame(rng, {1: 12 + 5 * k, 2: 8, 3: 5 + k})
        case("position_%d" % k, ls, ld, d, [(list(range(len(ls))), list(range(len(ld))), {1: 2.0, 2: 1.0, 3: 3.0})])
    ls, ld, d = riou_frame(rng, 30, 26)
    case("riou_ones", ls, ld, d, [(list(range(30)), list(range(26)), {0: 0.9, 1: 0.7})])
    ls, ld = rng.integers(0, 2, 24), rng.integers(0, 2, 20)
    d = (rng.integers(0, 8, (24, 20)) * 0.25).astype(np.float32)
    case("quantized", ls, ld, d, [(list(range(24)), list(range(20)), {0: 1.0, 1: 1.25})])
    d = (rng.integers(0, 4, (40, 40)) * 0.25).astype(np.float32)
    case("quantized_one_class", np.zeros(40), np.zeros(40), d, [(list(range(40)), list(range(40)), {0: 0.5})])
    case("constant", np.zeros(7), np.zeros(7), np.full((7, 7), 0.5, np.float32), [(list(range(7)), list(range(7)), {0: 1.0})])
    d = rng.random((9, 17)).astype(np.float32)
    case("wide", np.zeros(9), np.zeros(17), d, [(list(range(9)), list(range(17)), {0: 0.8})])
    d = (rng.integers(0, 5, (17, 9)) * 0.25).astype(np.float32)
    case("tall", np.zeros(17), np.zeros(9), d, [(list(range(17)), list(range(9)), {0: 0.75})])
    ls, ld, d = position_frame(rng, {1: 10, 2: 7})
    ss, ds = list(rng.permutation(len(ls))[:len(ls) - 2]), list(rng.permutation(len(ld))[:len(ld) - 1])
    case("unsorted_subsets", ls, ld, d, [([int(x) for x in ss], [int(x) for x in ds], {1: 2.0, 2: 2.0})])
    ls, ld, d = position_frame(rng, {1: 8, 2: 6})
    ls = ls.copy()
    ls[:3] = 5                                       # a source class without destinations
    case("class_without_dst", ls, ld, d, [(list(range(len(ls))), list(range(len(ld))), {1: 2.5, 2: 2.5, 5: 9.0})])
    ls, ld, d = position_frame(rng, {1: 8, 2: 6, 4: 5})
    case("tag_missing_from_thr", ls, ld, d, [(list(range(len(ls))), list(range(len(ld))), {1: 2.5, 2: 2.5})])
    d = np.array([[0.5, 0.75, 1.0], [0.5, 0.25, 0.75], [1.0, 0.5, 0.5]], np.float32)
    case("at_threshold", np.zeros(3), np.zeros(3), d, [(list(range(3)), list(range(3)), {0: 0.5})])
    ls, ld, d = position_frame(rng, {1: 9, 2: 6})
    n, m = len(ls), len(ld)
    case("two_calls", ls, ld, d, [(list(range(0, n, 2)), list(range(m)), {1: 1.5, 2: 1.5}),
                                  (list(range(n)), list(range(0, m, 2)) + list(range(1, m, 2)), {1: 3.0, 2: 3.0})])
    return out


LSAP_SHAPES = [(1, 1), (64, 64), (65, 65), (257, 300), (300, 257), (1000, 3000)]


def lsap_matrix(shape, seed):
    """tie-heavy: multiples of 0.25 in [0, 2), fp32"""
    return (np.random.default_rng(seed).integers(0, 8, shape) * 0.25).astype(np.float32)


def maps(mt, n, m):
    s = np.array([mt.query_src_match(i) for i in range(n)], np.int32)
    d = np.array([mt.query_dst_match(j) for j in range(m)], np.int32)
    return s, d


def main():
    d3d = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/d3d"
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(20261016)
    out, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        ref = build_reference(d3d, tmp)
        for name, ls, ld, dist, calls in cases(rng):
            n, m = dist.shape
            out[name + "/dist"], out[name + "/src_tags"], out[name + "/dst_tags"] = dist, ls, ld
            ties = any(np.unique(dist[np.ix_(s, d)]).size < len(s) * len(d) for s, d, _ in calls)
            meta[name] = dict(calls=[dict(src=[int(x) for x in s], dst=[int(x) for x in d],
                                          thr={str(k): float(v) for k, v in t.items()}) for s, d, t in calls], nn_ties=bool(ties))
            for kind, cls in (("hungarian", ref.HungarianMatcher), ("nn", ref.NearestNeighborMatcher)):
                mt = cls()
                mt.set_cache(ls.tolist(), ld.tolist(), dist)
                for k, (s, d, t) in enumerate(calls):
                    mt.match(s, d, {int(a): float(b) for a, b in t.items()})
                    out["%s/%s/%d/src" % (name, kind, k)], out["%s/%s/%d/dst" % (name, kind, k)] = maps(mt, n, m)
        for k, shape in enumerate(LSAP_SHAPES):
            c = lsap_matrix(shape, 1000 + k)
            a, b = linear_sum_assignment(c)
            key = "lsap/%dx%d" % shape
            out[key + "/rows"], out[key + "/cols"] = a.astype(np.int32), b.astype(np.int32)
            out[key + "/checksum"] = np.array([c.astype(np.float64).sum(), float((c * np.arange(c.size).reshape(shape) % 97).sum())])
            if c.size <= 65 * 65:
                out[key + "/cost"] = c
            meta[key] = dict(shape=list(shape), seed=1000 + k)
        # the reference's single-core time on a tracker-sized frame: 3 classes of 100-500 boxes, Position distances
        ls, ld, d = position_frame(np.random.default_rng(7), {1: 500, 2: 250, 3: 100})
        thr = {1: 2.0, 2: 1.0, 3: 3.0}
        for kind, cls in (("hungarian", ref.HungarianMatcher), ("nn", ref.NearestNeighborMatcher)):
            mt = cls()
            mt.set_cache(ls.tolist(), ld.tolist(), d)
            best = 1e9
            for _ in range(3):
                mt.clear_match()
                t0 = time.perf_counter()
                mt.match(list(range(len(ls))), list(range(len(ld))), thr)
                best = min(best, time.perf_counter() - t0)
            out["time/%s_tracker_frame_s" % kind] = np.array([best])
        meta["time"] = dict(frame=[len(ls), len(ld)], classes={1: 500, 2: 250, 3: 100})
    out["__meta__"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(os.path.join(HERE, "matcher_ref_cases.npz"), **out)


if __name__ == "__main__":
    main()
