"""Shared helpers of the tracking tests: the checker's dict stats as TrackingEvalStats, and comparisons."""
import json
import os
from enum import Enum

import numpy as np

from d3d_amd.benchmarks import TrackingEvalStats

COUNTS = ("ngt", "ndt", "tp", "fp", "fn", "id_switches", "fragments")
ACCS = ("acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var")


def to_stats(d, classes, T):
    """a track_reference.calc_stats dict -> TrackingEvalStats (tid maps -> sorted (tids, counts) arrays)"""
    st = TrackingEvalStats().initialize(classes, T)
    for k in COUNTS + ACCS:
        setattr(st, k, {c: (list(v) if isinstance(v, list) else v) for c, v in d[k].items()})
    for c in classes:
        tids = np.array(sorted(d["ngt_ids"][c]), np.uint64)
        st.ngt_ids[c] = (tids, np.array([d["ngt_ids"][c][int(t)] for t in tids], np.int64))
        for name in ("ngt_tracked", "ndt_ids"):
            maps = d[name][c]
            u = np.array(sorted(set().union(*[set(m) for m in maps])), np.uint64)
            cnt = np.array([[m.get(int(t), 0) for t in u] for m in maps], np.int64).reshape(T, len(u))
            getattr(st, name)[c] = (u, cnt)
    return st


def same_float(a, b, rtol=1e-5, atol=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.isclose(a, b, rtol=rtol, atol=atol, equal_nan=True)))


def assert_stats_equal(got, exp, classes, where="", rtol=1e-5, atol=1e-6):
    """got: TrackingEvalStats; exp: a checker dict or another TrackingEvalStats.  Counts exact, accuracies to fp32 rounding
    (the defaults: both sides on the same distance cache) or to the given tolerances."""
    e = exp if isinstance(exp, dict) else exp.__dict__
    for k in COUNTS:
        for c in classes:
            assert getattr(got, k)[c] == e[k][c], "%s %s[%s]: %s != %s" % (where, k, c, getattr(got, k)[c], e[k][c])
    for k in ACCS:
        for c in classes:
            assert same_float(getattr(got, k)[c], e[k][c], rtol, atol), "%s %s[%s]: %s != %s" % (where, k, c, getattr(got, k)[c], e[k][c])
    o = got.as_object()
    for name in ("ngt_tracked", "ndt_ids"):
        for c in classes:
            if isinstance(exp, dict):
                ref = [sorted(m) for m in exp[name][c]]
            else:
                ref = exp.as_object()[name][c]
            assert o[name][c] == ref, "%s %s[%s]" % (where, name, c)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_ref_cases.npz")
CASES = ("seq_a", "seq_b", "seq_c", "hand")


class Cls(Enum):                                   # the golden generator's class enum (tests/golden/make_track_golden.py)
    Car = 1
    Pedestrian = 2
    Cyclist = 3


def golden():
    return np.load(GOLDEN)


def golden_case(z, name):
    """-> (classes, params dict, list of frames (gt, dt, gt_tids, dt_tids))"""
    p = name + "/"
    classes = [int(c) for c in z[p + "classes"]]
    params = json.loads(str(z[p + "params"]))
    frames = [(z[p + "f%d/gt" % f], z[p + "f%d/dt" % f], z[p + "f%d/gt_tids" % f], z[p + "f%d/dt_tids" % f])
              for f in range(int(z[p + "frames"]))]
    return classes, params, frames


def golden_evaluator(cls, classes, params):
    ov = params["min_overlaps"]
    return cls([Cls(c) for c in classes], ov, pr_sample_count=params["T"], pr_sample_scale=params["scale"])


def golden_stats(z, name, f, classes, T, tracking):
    """the reference's per-frame stats of a golden frame: a checker-layout dict (tid maps as {tid: count})"""
    q = "%s/f%d/%s/" % (name, f, "track" if tracking else "det")
    d = {"ngt": {c: int(v) for c, v in zip(classes, z[q + "ngt"])}}
    names = ["ndt", "tp", "fp", "fn"] + (["id_switches", "fragments"] if tracking else [])
    for k in names:
        d[k] = {c: [int(x) for x in row] for c, row in zip(classes, z[q + k])}
    for k in ACCS:
        d[k] = {c: [float(x) for x in row] for c, row in zip(classes, z[q + k])}
    if tracking:
        d["ngt_ids"] = {c: {} for c in classes}
        for c, _, tid, n in z[q + "ngt_ids"]:
            d["ngt_ids"][int(c)][int(tid)] = int(n)
        for k in ("ngt_tracked", "ndt_ids"):
            d[k] = {c: [dict() for _ in range(T)] for c in classes}
            for c, t, tid, n in z[q + k]:
                d[k][int(c)][int(t)][int(tid)] = int(n)
    return d


def plain(x):
    """metric results with Enum keys -> the golden JSON's layout (str(class value) keys)"""
    if isinstance(x, dict):
        return {str(k.value if isinstance(k, Enum) else k): plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def assert_json_close(got, exp, where):
    if isinstance(exp, dict):
        assert set(got) == set(exp), where
        for k in exp:
            assert_json_close(got[k], exp[k], "%s.%s" % (where, k))
    elif isinstance(exp, list):
        assert len(got) == len(exp), where
        for i, (a, b) in enumerate(zip(got, exp)):
            assert_json_close(a, b, "%s[%d]" % (where, i))
    elif isinstance(exp, float):
        assert same_float(got, exp, rtol=1e-6, atol=1e-7), "%s: %r != %r" % (where, got, exp)
    else:
        assert got == exp, "%s: %r != %r" % (where, got, exp)


def assert_summary_equal(got, exp):
    """the same lines; the classes' order is the reference's unordered_set order there, the given order here"""
    assert sorted(got.split("\n")) == sorted(exp.split("\n")), "\n%s\n----\n%s" % (got, exp)
