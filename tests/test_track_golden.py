"""CPU tests against tests/golden/track_ref_cases.npz (the reference's own DetectionEvaluator / TrackingEvaluator, compiled by
tests/golden/make_track_golden.py): the literal checker frame by frame, and add_stats plus every metric method of both
evaluators fed the reference's per-frame stats, against the reference's accumulated results."""
import json

import numpy as np
import pytest

import track_reference as tr
from track_cases import (CASES, assert_json_close, assert_stats_equal, assert_summary_equal, golden, golden_case,
                         golden_evaluator, golden_stats, plain, to_stats)
from d3d_amd.benchmarks import DetectionEvaluator, TrackingEvaluator
from d3d_amd.utils import Dict


@pytest.fixture(scope="module")
def z():
    return golden()


def _tolist(x):
    return x.tolist() if isinstance(x, np.ndarray) else x


@pytest.mark.parametrize("name", CASES)
def test_checker_against_golden(z, name):
    classes, params, frames = golden_case(z, name)
    ev = golden_evaluator(TrackingEvaluator, classes, params)
    md = {c: np.float32(v) for c, v in ev._max_distance.items()}
    st = tr.State(params["T"])
    for f, fr in enumerate(frames):
        got = tr.calc_stats(st, *fr, classes, md, ev.score_thresholds)
        exp = golden_stats(z, name, f, classes, params["T"], True)
        for k in ("ngt", "ndt", "tp", "fp", "fn", "id_switches", "fragments", "ngt_ids", "ngt_tracked", "ndt_ids"):
            assert got[k] == exp[k], "frame %d %s" % (f, k)
        for k in ("acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var"):
            for c in classes:
                assert np.allclose(got[k][c], exp[k][c], rtol=1e-5, atol=1e-6, equal_nan=True), "frame %d %s" % (f, k)


def _check_metrics(ev, exp, tracking):
    nan = float("nan")
    assert_json_close(plain(ev.gt_count()), exp["gt_count"], "gt_count")
    assert_json_close(plain(ev.ap()), exp["ap"], "ap")
    for name, kw in (("fscore", {}), ("precision", {}), ("recall", {})):
        assert_json_close(plain(getattr(ev, name)(return_all=True)), exp[name + "_all"], name + "_all")
    names = ["dt_count", "tp", "fp", "fn", "precision", "recall", "fscore", "acc_iou", "acc_box", "acc_dist", "acc_angular"]
    if tracking:
        names += ["id_switches", "fragments", "mota", "tracked_ratio", "lost_ratio"]
    for s, key in ((nan, "nan"), (0.0, "0"), (0.35, "0.35"), (0.8, "0.8")):
        for name in names:
            assert_json_close(plain(getattr(ev, name)(s)), exp["%s@%s" % (name, key)], "%s@%s" % (name, key))
    assert_summary_equal(ev.summary(), exp["summary"])
    assert_summary_equal(ev.summary(verbose=True), exp["summary_verbose"])
    if tracking:
        assert_json_close(plain(ev.gt_traj_count()), exp["gt_traj_count"], "gt_traj_count")
        assert_json_close(plain(ev.tracked_ratio(return_all=True)), exp["tracked_ratio_all"], "tracked_ratio_all")
        assert_json_close(plain(ev.lost_ratio(0.5, 0.3, return_all=True)), exp["lost_ratio_all"], "lost_ratio_all")
        assert_summary_equal(ev.summary(0.5, 0.7, 0.3, note="golden", verbose=True), exp["summary_note"])


@pytest.mark.parametrize("name", CASES)
def test_tracking_metrics_against_golden(z, name):
    classes, params, frames = golden_case(z, name)
    ev = golden_evaluator(TrackingEvaluator, classes, params)
    for f in range(len(frames)):
        ev.add_stats(to_stats(golden_stats(z, name, f, classes, params["T"], True), classes, params["T"]))
    _check_metrics(ev, json.loads(str(z[name + "/track_metrics"])), True)


@pytest.mark.parametrize("name", CASES)
def test_detection_metrics_against_golden(z, name):
    classes, params, frames = golden_case(z, name)
    ev = golden_evaluator(DetectionEvaluator, classes, params)
    for f in range(len(frames)):
        ev.add_stats(Dict(golden_stats(z, name, f, classes, params["T"], False)))
    _check_metrics(ev, json.loads(str(z[name + "/det_metrics"])), False)


def test_golden_records_reference_time(z):
    assert float(z["time/frame_100x150_s"][0]) > 0
