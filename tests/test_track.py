"""CPU tests of TrackingEvaluator / TrackingEvalStats and the detection evaluator's accumulation API: the host code (add_stats,
every metric, constructor errors, tid validation, as_object, pickling) against the literal checker of tests/track_reference.py."""
import math
import pickle
from enum import Enum

import numpy as np
import pytest

import track_reference as tr
from track_cases import assert_stats_equal, to_stats
from d3d_amd import synth
from d3d_amd.benchmarks import DetectionEvaluator, TrackingEvalStats, TrackingEvaluator

CLASSES = [1, 2]


class Obj(Enum):
    Car = 1
    Pedestrian = 2


def _checker_sequence(ev, seed, frames=6):
    g, d, gi, di, go, do = synth.tracking_sequence(frames=frames, n_tracks=12, seed=seed)
    md = {c: np.float32(v) for c, v in ev._max_distance.items()}
    st = tr.State(ev._pr_nsamples)
    return [tr.calc_stats(st, g[go[f]:go[f + 1]], d[do[f]:do[f + 1]], gi[go[f]:go[f + 1]], di[do[f]:do[f + 1]],
                          ev._classes, md, ev.score_thresholds) for f in range(frames)]


@pytest.fixture(scope="module")
def frames():
    ev = TrackingEvaluator(CLASSES, 0.5, pr_sample_count=12)
    return _checker_sequence(ev, seed=3)


def test_checker_sequence_is_consistent(frames):
    for s in frames:
        for c in CLASSES:
            assert [a + b for a, b in zip(s["tp"][c], s["fn"][c])] == [s["ngt"][c]] * 12
            assert s["ndt"][c] == [len(m) for m in s["ndt_ids"][c]]
            assert s["tp"][c] == [len(m) for m in s["ngt_tracked"][c]]
    assert sum(sum(s["id_switches"][c]) for s in frames for c in CLASSES) > 0
    assert sum(sum(s["fragments"][c]) for s in frames for c in CLASSES) > 0


@pytest.mark.parametrize("typed", [False, True])
def test_add_stats_and_metrics_match_checker(frames, typed):
    ev = TrackingEvaluator([Obj.Car, Obj.Pedestrian] if typed else CLASSES, 0.5, pr_sample_count=12)
    acc = tr.Accumulator(CLASSES, ev.score_thresholds)
    for s in frames:
        ev.add_stats(to_stats(s, CLASSES, 12))
        acc.add(s)
    key = (lambda c: Obj(c)) if typed else (lambda c: c)
    got = ev.get_stats()
    assert_stats_equal(got, acc.s, CLASSES)
    for c in CLASSES:
        assert got.as_object()["ngt_ids"][c] == sorted(acc.s["ngt_ids"][c])
        gids, gcnt = got.ngt_ids[c]
        assert {int(t): int(n) for t, n in zip(gids, gcnt)} == acc.s["ngt_ids"][c]
    for score in (math.nan, 0.0, 0.3, 0.5, 0.8):
        i = acc.idx(score)
        assert ev._get_score_idx(score) == i
        for name in ("tp", "fp", "fn", "ndt", "id_switches", "fragments"):
            m = getattr(ev, "dt_count" if name == "ndt" else name)(score)
            assert m == {key(c): acc.s[name][c][i] for c in CLASSES}, name
        assert ev.precision(score) == {key(c): v for c, v in acc.precision(i).items()}
        assert ev.recall(score) == {key(c): v for c, v in acc.recall(i).items()}
        assert ev.mota(score) == pytest.approx({key(c): v for c, v in acc.mota(i).items()})
        assert ev.tracked_ratio(score) == {key(c): v for c, v in acc.frame_ratio(i, 0.8, True).items()}
        assert ev.lost_ratio(score) == {key(c): v for c, v in acc.frame_ratio(i, 0.2, False).items()}
        for name in ("acc_iou", "acc_box", "acc_dist", "acc_angular"):
            got_v, exp_v = getattr(ev, name)(score), acc.s[name]
            for c in CLASSES:
                assert np.isclose(got_v[key(c)], exp_v[c][i], rtol=1e-5, equal_nan=True)
    assert ev.ap() == pytest.approx({key(c): v for c, v in acc.ap().items()})
    assert ev.tracked_ratio(return_all=True)[key(1)] == [acc.frame_ratio(i, 0.8, True)[1] for i in range(12)]
    assert len(ev.fscore(return_all=True)[key(2)]) == 12
    assert ev.gt_count() == {key(c): acc.s["ngt"][c] for c in CLASSES}
    assert ev.gt_traj_count() == {key(c): len(acc.s["ngt_ids"][c]) for c in CLASSES}
    text = ev.summary(verbose=True)
    assert ("Car" in text) == typed and "MOTA" in text and "mAP" in text
    short = ev.summary(note="seq")
    assert "Benchmark Summary (seq)" in short and ("Results for %s:" % ("Car" if typed else "1")) in short


def test_detection_evaluator_accumulation():
    """DetectionEvaluator.add_stats / metrics on the detection part of the checker's stats"""
    ev = DetectionEvaluator([Obj.Car, Obj.Pedestrian], [0.5, 0.7], pr_sample_count=12)
    tev = TrackingEvaluator([Obj.Car, Obj.Pedestrian], [0.5, 0.7], pr_sample_count=12)
    acc = tr.Accumulator(CLASSES, ev.score_thresholds)
    for s in _checker_sequence(tev, seed=5, frames=4):
        det = {k: s[k] for k in ("ngt", "ndt", "tp", "fp", "fn", "acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var")}
        from d3d_amd.utils import Dict
        ev.add_stats(Dict(det))
        acc.add(dict(s))
    st = ev.get_stats()
    for c in CLASSES:
        assert st.tp[c] == acc.s["tp"][c] and st.fp[c] == acc.s["fp"][c] and st.ngt[c] == acc.s["ngt"][c]
        assert np.allclose(st.acc_iou[c], acc.s["acc_iou"][c], equal_nan=True)
    assert ev.ap() == pytest.approx({Obj(c): v for c, v in acc.ap().items()})
    assert set(ev.tp()) == {Obj.Car, Obj.Pedestrian}
    assert "Results for Car" in ev.summary()
    ev.reset()
    assert ev.get_stats().tp[1] == [0] * 12 and math.isnan(ev.get_stats().acc_iou[1][0])


def test_wmean_fp32():
    ev = DetectionEvaluator([1], 0.5, pr_sample_count=2)
    one = dict(ngt={1: 1}, ndt={1: [1, 1]}, tp={1: [1, 0]}, fp={1: [0, 1]}, fn={1: [0, 1]},
               acc_iou={1: [0.1, math.nan]}, acc_angular={1: [0.2, math.nan]}, acc_dist={1: [0.3, math.nan]},
               acc_box={1: [0.4, math.nan]}, acc_var={1: [-math.inf, math.nan]})
    from d3d_amd.utils import Dict
    ev.add_stats(Dict(one))
    two = dict(one, tp={1: [2, 0]}, acc_iou={1: [0.7, math.nan]})
    ev.add_stats(Dict(two))
    exp = float((np.float32(0.1) * np.float32(1) + np.float32(0.7) * np.float32(2)) / np.float32(3))
    assert ev.get_stats().acc_iou[1][0] == exp
    assert math.isnan(ev.get_stats().acc_iou[1][1])
    assert ev.get_stats().acc_var[1][0] == -math.inf


def test_constructor_errors():
    with pytest.raises(ValueError):
        TrackingEvaluator([1], "0.5")
    with pytest.raises(ValueError):
        TrackingEvaluator([1], 0.5, pr_sample_scale="quad")
    with pytest.raises(AssertionError):
        TrackingEvaluator([], 0.5)
    ev = TrackingEvaluator(Obj.Car, 0.7, pr_sample_count=10, pr_sample_scale="lin", min_score=0.1)
    assert ev._classes == [1] and len(ev.score_thresholds) == 10 and ev.score_thresholds[0] == np.float32(0.1)
    assert ev._max_distance[1] == pytest.approx(0.3)


def test_tid_validation():
    ev = TrackingEvaluator(CLASSES, 0.5, pr_sample_count=4)
    gt = np.zeros((2, 9), np.float32)
    gt[:, 0] = 1
    dt = gt.copy()
    dt[:, 1] = 0.9
    ok = np.array([1, 2], np.uint64)
    with pytest.raises(ValueError):
        ev.calc_stats(gt, dt, np.array([3, 3], np.uint64), ok)
    with pytest.raises(ValueError):
        ev.calc_stats(gt, dt, ok, np.array([5, 5], np.int64))
    with pytest.raises(AssertionError):
        ev.calc_stats(gt, dt, ok, np.array([0, 1], np.uint64))
    with pytest.raises(ValueError):
        ev.calc_stats(gt, dt, ok, np.array([1, 2], np.int32))
    with pytest.raises(ValueError):
        ev.calc_stats(gt, dt, ok, np.array([1], np.uint64))
    dt[0, 0] = 7                                     # tid 0 outside `classes` / below every threshold: not selected, fine
    dt[1, 1] = -1
    h = ev._prepare_host(gt, dt, ok, np.array([0, 9], np.uint64))
    assert not h["sel"].any() and list(h["row_off"]) == [0] * 5
    with pytest.raises(ValueError):
        ev.calc_stats_sequence(gt, dt, ok, ok, [0, 1], [0, 2])
    with pytest.raises(ValueError):
        ev.calc_stats_sequence(gt, dt, ok, ok, [0, 2], [0, 1, 2])


def test_as_object_layout_and_pickle(frames):
    st = to_stats(frames[2], CLASSES, 12)
    o = st.as_object()
    assert set(o) == {"ngt", "tp", "fp", "fn", "ndt", "acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var",
                      "id_switches", "fragments", "ngt_ids", "ngt_tracked", "ndt_ids"}
    assert isinstance(o["ngt_ids"][1], list) and len(o["ngt_tracked"][1]) == 12 and len(o["ndt_ids"][2]) == 12
    assert o["ngt_ids"][1] == sorted(frames[2]["ngt_ids"][1])
    st2 = pickle.loads(pickle.dumps(st))
    assert_stats_equal(st2, st, CLASSES)
    assert st2.as_object()["ngt_ids"] == o["ngt_ids"]
    ev = TrackingEvaluator(CLASSES, 0.5, pr_sample_count=12)
    ev.add_stats(st)
    ev2 = pickle.loads(pickle.dumps(ev))
    assert_stats_equal(ev2.get_stats(), ev.get_stats(), CLASSES)
    ev2.reset()
    assert ev2.get_stats().as_object()["ngt_ids"] == {1: [], 2: []}
