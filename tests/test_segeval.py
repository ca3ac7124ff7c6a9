"""CPU: SegmentationEvaluator / SegmentationStats (reference d3d/benchmarks.pyx:891-1213) without a GPU -- the checker against the
reference's goldens, the constructor's parsing and errors, the host bookkeeping, pickling, the workspace query."""
import math
import os
import pickle
from enum import Enum

import numpy as np
import pytest

import seg_reference

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("tp", "fp", "fn", "itp", "ifp", "ifn")


def golden_cases():
    z = np.load(os.path.join(HERE, "golden", "seg_ref_cases.npz"))
    names = sorted({k.split("/")[0] for k in z.files if k.startswith("c")}, key=lambda s: int(s[1:]))
    for c in names:
        p = c + "/"
        yield dict(classes=z[p + "classes"].tolist(), background=int(z[p + "params"][0]), min_points=int(z[p + "params"][1]),
                   gt_labels=z[p + "gt_labels"], pred_labels=z[p + "pred_labels"],
                   gt_ids=z[p + "gt_ids"] if p + "gt_ids" in z.files else None,
                   pred_ids=z[p + "pred_ids"] if p + "pred_ids" in z.files else None,
                   counts=z[p + "counts"], cumiou=z[p + "cumiou"], name=c)


def as_arrays(stats):
    """as_object()-style dicts -> counts [6, 256], cumiou [256]"""
    counts = np.zeros((6, 256), np.int64)
    cum = np.zeros((256,), np.float32)
    for i, f in enumerate(FIELDS):
        for k, v in stats[f].items():
            counts[i, k] = v
    for k, v in stats["cumiou"].items():
        cum[k] = v
    return counts, cum


def test_goldens_cover_the_cases():
    cases = list(golden_cases())
    assert len(cases) >= 64
    pano = [c for c in cases if c["gt_ids"] is not None]
    assert len(pano) == len(cases) // 2
    tot = sum(c["counts"] for c in pano)
    assert tot[3].sum() > 0 and tot[4].sum() > 0 and tot[5].sum() > 0      # matches, unmatched predictions and ground truths
    assert any(c["background"] in c["classes"] or 256 + c["background"] in c["classes"] for c in cases)
    assert any(c["background"] not in c["classes"] for c in cases)
    assert len({c["min_points"] for c in cases}) >= 4


def test_checker_equals_every_golden_case():
    for c in golden_cases():
        bg = c["background"] if c["background"] >= 0 else 256 + c["background"]
        got = seg_reference.calc_stats(c["classes"], bg, c["min_points"], c["gt_labels"], c["pred_labels"], c["gt_ids"], c["pred_ids"])
        counts, cum = as_arrays(got)
        assert np.array_equal(counts, c["counts"]), c["name"]
        np.testing.assert_allclose(cum, c["cumiou"], rtol=1e-5, err_msg=c["name"])


class Cls(Enum):
    UNLABELED = 0
    CAR = 1
    PERSON = 2
    ROAD = 9


def test_constructor_parsing_and_errors():
    from d3d_amd.benchmarks import SegmentationEvaluator
    ev = SegmentationEvaluator([Cls.CAR, Cls.PERSON], background=Cls.UNLABELED)
    assert ev._classes == [1, 2] and ev._class_type is Cls and ev._background == 0
    assert set(ev.tp()) == {Cls.CAR, Cls.PERSON} and set(ev.iou(instance=True)) == {Cls.CAR, Cls.PERSON}
    ev = SegmentationEvaluator(3, background=-1, min_points=7)
    assert ev._classes == [3] and ev._background == 255 and ev._min_points == 7 and ev._class_type is None
    assert SegmentationEvaluator((4, 5), background=-256)._background == 0
    assert ev._mask == (8,) + (0,) * 7
    assert SegmentationEvaluator([255, 0, 32])._mask == (1, 1) + (0,) * 5 + (1 << 31,)
    with pytest.raises(ValueError, match="255 different categories"):
        SegmentationEvaluator(list(range(256)))
    SegmentationEvaluator(list(range(255)))
    with pytest.raises(ValueError, match="int or Enum"):
        SegmentationEvaluator(["car"])
    with pytest.raises(OverflowError):
        SegmentationEvaluator([256])
    with pytest.raises(AssertionError):
        SegmentationEvaluator([])
    labels = np.zeros((10,), np.uint8)
    for bad in (np.zeros((10,), np.int32), np.zeros((10,), np.int16), [0] * 10):
        with pytest.raises(ValueError, match="Please convert ids to uint16!"):
            ev.calc_stats(labels, labels, bad, np.zeros((10,), np.uint16))
        with pytest.raises(ValueError, match="Please convert ids to uint16!"):
            ev.calc_stats(labels, labels, np.zeros((10,), np.uint16), bad)


def hand_stats(classes, **fields):
    from d3d_amd.benchmarks import SegmentationStats
    s = SegmentationStats()
    s.initialize(classes)
    for name, vals in fields.items():
        getattr(s, name).update(vals)
    return s


def test_bookkeeping_on_hand_built_stats():
    from d3d_amd.benchmarks import SegmentationEvaluator, SegmentationStats
    ev = SegmentationEvaluator([0, 1, 2, 3])
    a = hand_stats([0, 1, 2, 3], tp={1: 6, 2: 1}, fp={1: 2, 2: 0}, fn={1: 1, 2: 3}, itp={1: 2, 2: 0}, ifp={1: 1, 2: 2},
                   ifn={1: 0, 2: 1}, cumiou={1: 1.5, 2: 0.0})
    b = hand_stats([0, 1, 2, 3], tp={1: 1}, fp={2: 1}, itp={1: 1}, cumiou={1: 0.7})
    ev.add_stats(a)
    ev.add_stats(b)
    s = ev.get_stats()
    assert isinstance(s, SegmentationStats)
    assert s.tp == {0: 0, 1: 7, 2: 1, 3: 0} and s.fp == {0: 0, 1: 2, 2: 1, 3: 0} and s.fn == {0: 0, 1: 1, 2: 3, 3: 0}
    assert s.itp[1] == 3 and s.ifp[2] == 2 and s.ifn[2] == 1
    assert s.cumiou[1] == float(np.float32(np.float32(1.5) + np.float32(0.7)))
    assert ev.tp() == s.tp and ev.tp(instance=True) == s.itp and ev.fp(True) == s.ifp and ev.fn(True) == s.ifn
    iou = ev.iou()
    assert iou[1] == float(np.float32(7) / np.float32(10)) and iou[2] == float(np.float32(1) / np.float32(5))
    assert math.isnan(iou[0]) and math.isnan(iou[3])
    sq = ev.sq()
    assert sq[1] == float(np.float32(s.cumiou[1]) / np.float32(3)) and math.isnan(sq[2]) and math.isnan(sq[0])
    rq = ev.rq()
    assert rq[1] == float(np.float32(3) / np.float32(3.5)) and rq[2] == 0.0 and math.isnan(rq[3])
    pq = ev.pq()
    assert pq[1] == sq[1] * rq[1] and math.isnan(pq[2])
    text = ev.summary()
    lines = text.split("\n")
    assert lines[0] == "========== Benchmark Summary ==========" and lines[-1] == "========== Summary End =========="
    assert "   0:" not in text                                                # the background is left out
    assert lines[1] == "   1: iou=%.3f, sq=%.3f, rq=%.3f, pq=%.3f" % (iou[1], sq[1], rq[1], pq[1])
    assert lines[2] == "   2: iou=%.3f" % iou[2] and lines[3] == "   3: iou=nan"
    assert "mean IoU: %.4f" % ((iou[1] + iou[2]) / 2) in lines and "mean PQ: %.4f" % pq[1] in lines
    ev.reset()
    assert ev.get_stats().tp == {0: 0, 1: 0, 2: 0, 3: 0} and all(math.isnan(v) for v in ev.iou().values())
    assert "mean SQ" not in ev.summary() and "mean IoU: nan" in ev.summary()


def test_enum_keyed_results_and_summary_names():
    from d3d_amd.benchmarks import SegmentationEvaluator
    ev = SegmentationEvaluator([Cls.UNLABELED, Cls.CAR, Cls.ROAD])
    ev.add_stats(hand_stats([0, 1, 9], tp={1: 3, 9: 4}, fn={1: 1}, itp={9: 1}, cumiou={9: 0.75}))
    assert ev.tp() == {Cls.UNLABELED: 0, Cls.CAR: 3, Cls.ROAD: 4} and ev.fn()[Cls.CAR] == 1
    assert ev.iou()[Cls.CAR] == 0.75 and ev.sq()[Cls.ROAD] == 0.75 and ev.rq()[Cls.ROAD] == 1.0
    assert set(ev.pq()) == {Cls.UNLABELED, Cls.CAR, Cls.ROAD}
    text = ev.summary()
    assert "                 CAR: iou=0.750" in text and "                ROAD: iou=1.000, sq=0.750, rq=1.000, pq=0.750" in text
    assert "UNLABELED" not in text


def test_pickle_round_trip():
    from d3d_amd.benchmarks import SegmentationEvaluator, SegmentationStats
    s = hand_stats([1, 2], tp={1: 5}, itp={2: 1}, cumiou={2: 0.625})
    s2 = pickle.loads(pickle.dumps(s))
    assert isinstance(s2, SegmentationStats) and s2 == s and s2.as_object() == s.as_object()
    assert s.as_object() == dict(tp={1: 5, 2: 0}, fp={1: 0, 2: 0}, fn={1: 0, 2: 0}, itp={1: 0, 2: 1}, ifp={1: 0, 2: 0},
                                 ifn={1: 0, 2: 0}, cumiou={1: 0.0, 2: 0.625})
    ev = SegmentationEvaluator([Cls.CAR, Cls.PERSON], background=Cls.UNLABELED, min_points=4)
    ev.add_stats(hand_stats([1, 2], tp={1: 2}, fp={2: 1}))
    ev2 = pickle.loads(pickle.dumps(ev))
    assert ev2.get_stats() == ev.get_stats() and ev2.summary() == ev.summary()
    assert ev2._min_points == 4 and ev2._mask == ev._mask and ev2._class_type is Cls


def test_segeval_workspace_query_is_pure():
    from d3d_amd import _lib
    lib = _lib.load()
    a = lib.d3d_segeval_workspace_bytes(120000, 1)
    assert a == lib.d3d_segeval_workspace_bytes(120000, 1)          # no state
    assert a >= 3 * 12 * 120000 and a < 64 * 120000                    # three tables of 12-byte slots, load <= 0.8
    assert lib.d3d_segeval_workspace_bytes(120000, 100) - a == d3d_align(100 * 256 * 8) - d3d_align(256 * 8)   # + [F, 256] u64 sums
    assert lib.d3d_segeval_workspace_bytes(0, 0) > 0 and lib.d3d_segeval_workspace_bytes(-1, 1) == 0
    assert lib.d3d_segeval_workspace_bytes(8 << 20, 1) > lib.d3d_segeval_workspace_bytes(1 << 20, 1)


def d3d_align(x):
    return (x + 255) // 256 * 256


def test_segeval_rejects_bad_arguments_without_launching():
    """argument checks come before any device work: a NULL stream / workspace is never touched"""
    import ctypes
    from d3d_amd import _lib
    lib = _lib.load()
    mask = (ctypes.c_uint32 * 8)(2, 0, 0, 0, 0, 0, 0, 0)
    nul = [None] * 7

    def call(n, frames, gi=None, pi=None, bg=0, m=mask):
        return lib.d3d_segeval(None, None, gi, pi, None, n, frames, m, bg, 0, *nul, None, 0, None)
    assert call(0, 0) == _lib.OK                                       # nothing to do
    assert call(10, 0) == _lib.ERR_BAD_ARG                             # points without frames
    assert call(0, 65536) == _lib.ERR_BAD_ARG
    assert call(0, 1, bg=256) == _lib.ERR_BAD_ARG
    assert call(0, 1, gi=ctypes.c_void_p(16)) == _lib.ERR_BAD_ARG     # one id array only
    assert call(0, 1, m=None) == _lib.ERR_BAD_ARG
    assert call(0, 1) == _lib.ERR_BAD_ARG                              # missing outputs
