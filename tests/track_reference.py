"""A literal restatement of TrackingEvaluator.calc_stats / add_stats and its metrics (reference d3d/benchmarks.pyx:536-890) in
Python on top of oracle.prepare_boxes / oracle.score_match(literal=True): the checker of the GPU path.

Frames are [n,9] arrays plus uint64 track ids.  The carried state is a `State` (the reference's _last_* maps per threshold);
calc_stats returns a dict in the layout of TrackingEvalStats with the tid maps as plain {tid: count} dicts.  Counts under a
class outside `classes` are dropped (the reference indexes a missing map entry there)."""
import math

import numpy as np

import oracle


class State:
    def __init__(self, T):
        self.gt = [dict() for _ in range(T)]          # _last_gt_assignment: gt_tid -> dt_tid
        self.dt = [dict() for _ in range(T)]          # _last_dt_assignment: dt_tid -> gt_tid
        self.gt_tags = [dict() for _ in range(T)]
        self.dt_tags = [dict() for _ in range(T)]


def _wyaw(a, b):
    d = np.float32(a) - np.float32(b)
    return float(np.abs((d + np.pi) % (2 * np.pi) - np.pi) / np.pi)


def calc_stats(state, gt, dt, gt_tids, dt_tids, classes, max_distance, thresholds, cache=None):
    """:536-723 as written.  max_distance: {class: fp32 distance}; cache: the [n, m] distance matrix (default: the oracle's)"""
    T = len(thresholds)
    gt = np.asarray(gt, np.float32).reshape(-1, 9)
    dt = np.asarray(dt, np.float32).reshape(-1, 9)
    gt_tids = [int(x) for x in np.asarray(gt_tids, np.uint64)]
    dt_tids = [int(x) for x in np.asarray(dt_tids, np.uint64)]
    if cache is None:
        cache = oracle.prepare_boxes(dt, gt)
    cache = np.asarray(cache, np.float32)
    cls = set(classes)
    md = {c: float(np.float32(v)) for c, v in max_distance.items()}
    s = dict(ngt={c: 0 for c in classes}, ndt={c: [0] * T for c in classes}, tp={c: [0] * T for c in classes},
             fp={c: [0] * T for c in classes}, fn={c: [0] * T for c in classes},
             id_switches={c: [0] * T for c in classes}, fragments={c: [0] * T for c in classes},
             ngt_ids={c: {} for c in classes}, ngt_tracked={c: [dict() for _ in range(T)] for c in classes},
             ndt_ids={c: [dict() for _ in range(T)] for c in classes})
    acc = {k: [dict() for _ in range(T)] for k in ("iou", "angular", "dist", "box")}

    def add(table, tag, t, v=1):
        if tag in cls:
            table[tag][t] += v

    gtag = [int(x) for x in gt[:, 0]]
    dtag = [int(x) for x in dt[:, 0]]
    gt_indices, gt_tid_set = [], set()
    for g in range(len(gt)):                                                     # :575-584
        if gtag[g] not in cls:
            continue
        s["ngt"][gtag[g]] += 1
        s["ngt_ids"][gtag[g]][gt_tids[g]] = 1
        gt_tid_set.add(gt_tids[g])
        gt_indices.append(g)
    for t in range(T):
        thr = np.float32(thresholds[t])
        gt_asg, dt_asg = {}, {}                                                  # tid -> idx
        dt_indices, dt_tid_set = [], set()
        for d in range(len(dt)):                                                 # :588-614
            if dtag[d] not in cls or dt[d, 1] < thr:
                continue
            tid = dt_tids[d]
            assert tid > 0, "Tracking id should be greater than 0 for a valid object!"
            dt_tid_set.add(tid)
            s["ndt"][dtag[d]][t] += 1
            s["ndt_ids"][dtag[d]][t][tid] = 1
            if tid not in state.dt[t]:
                dt_indices.append(d)
            else:
                g_tid = state.dt[t][tid]
                for g in range(len(gt)):
                    if g_tid == gt_tids[g]:
                        if cache[d, g] > md[dtag[d]]:
                            dt_indices.append(d)
                        else:
                            gt_asg[g_tid] = d
                            dt_asg[tid] = g
                        break
        sa, da = oracle.score_match(cache, dt, gt, dt_indices, gt_indices, md, literal=True)   # :617-618
        for g in gt_indices:                                                     # :620-660
            g_tid = gt_tids[g]
            d = da.get(g, -1)
            if d >= 0:
                if g_tid in gt_asg:
                    del dt_asg[dt_tids[gt_asg[g_tid]]]
                    add(s["fp"], dtag[d], t)
                gt_asg[g_tid] = d
                dt_asg[dt_tids[d]] = g
            if g_tid not in gt_asg:
                s["fn"][gtag[g]][t] += 1
                continue
            d = gt_asg[g_tid]
            s["tp"][gtag[g]][t] += 1
            s["ngt_tracked"][gtag[g]][t][g_tid] = 1
            acc["iou"][t][g] = float(np.float32(1) - cache[d, g])
            dp, db = gt[g, 2:5] - dt[d, 2:5], gt[g, 5:8] - dt[d, 5:8]
            acc["dist"][t][g] = float(np.sqrt(np.sum(dp * dp)))
            acc["box"][t][g] = float(np.sqrt(np.sum(db * db)))
            acc["angular"][t][g] = _wyaw(gt[g, 8], dt[d, 8])
        for d in dt_indices:                                                     # :662-666
            if dt_tids[d] not in dt_asg:
                add(s["fp"], dtag[d], t)
        for g_tid, d_tid in state.gt[t].items():                                 # :668-676
            tag = state.gt_tags[t][g_tid]
            if g_tid not in gt_asg:
                if g_tid in gt_tid_set:
                    add(s["id_switches"], tag, t)
            elif dt_tids[gt_asg[g_tid]] != d_tid:
                add(s["id_switches"], tag, t)
        for d_tid, g_tid in state.dt[t].items():                                 # :678-685
            tag = state.dt_tags[t][d_tid]
            if d_tid not in dt_asg:
                if d_tid in dt_tid_set:
                    add(s["fragments"], tag, t)
            elif gt_tids[dt_asg[d_tid]] != g_tid:
                add(s["fragments"], tag, t)
        state.gt[t], state.dt[t], state.gt_tags[t], state.dt_tags[t] = {}, {}, {}, {}
        for g_tid, d in gt_asg.items():                                          # :687-703
            d_tid = dt_tids[d]
            g = dt_asg.get(d_tid, 0)                                             # operator[]
            state.gt[t][g_tid] = d_tid
            state.dt[t][d_tid] = g_tid
            state.gt_tags[t][g_tid] = gtag[g]
            state.dt_tags[t][d_tid] = dtag[d]
    for name, per_t in acc.items():                                              # _aggregate_stats (:155-176)
        out = {c: [math.nan] * T for c in classes}
        for t in range(T):
            for c in classes:
                vals = [v for g, v in per_t[t].items() if gtag[g] == c]
                if vals:
                    out[c][t] = float(np.float32(np.sum(np.asarray(vals, np.float64)) / len(vals)))
        s["acc_" + name] = out
    s["acc_var"] = {c: [-math.inf if s["tp"][c][t] else math.nan for t in range(T)] for c in classes}
    return s


def _wmean(a, wa, b, wb):
    if wa == 0:
        return b
    if wb == 0:
        return a
    return float((np.float32(a) * np.float32(wa) + np.float32(b) * np.float32(wb)) / np.float32(wa + wb))


class Accumulator:
    """add_stats (:300-327, :725-756) and the metrics (:329-447, :758-890) over dict stats, the reference's loops"""

    def __init__(self, classes, thresholds):
        self.classes, self.thr, T = list(classes), np.asarray(thresholds, np.float32), len(thresholds)
        self.T = T
        self.s = dict(ngt={c: 0 for c in classes})
        for k in ("ndt", "tp", "fp", "fn", "id_switches", "fragments"):
            self.s[k] = {c: [0] * T for c in classes}
        for k in ("acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var"):
            self.s[k] = {c: [math.nan] * T for c in classes}
        self.s["ngt_ids"] = {c: {} for c in classes}
        self.s["ngt_tracked"] = {c: [dict() for _ in range(T)] for c in classes}
        self.s["ndt_ids"] = {c: [dict() for _ in range(T)] for c in classes}

    def add(self, st):
        s = self.s
        for k in self.classes:
            s["ngt"][k] += st["ngt"][k]
            for i in range(self.T):
                otp, ntp = s["tp"][k][i], st["tp"][k][i]
                for name in ("acc_angular", "acc_box", "acc_iou", "acc_dist", "acc_var"):
                    s[name][k][i] = _wmean(s[name][k][i], otp, st[name][k][i], ntp)
                for name in ("ndt", "tp", "fp", "fn", "id_switches", "fragments"):
                    s[name][k][i] += st[name][k][i]
                for name in ("ngt_tracked", "ndt_ids"):
                    for tid, c in st[name][k][i].items():
                        s[name][k][i][tid] = s[name][k][i].get(tid, 0) + c
            for tid, c in st["ngt_ids"][k].items():
                s["ngt_ids"][k][tid] = s["ngt_ids"][k].get(tid, 0) + c

    def idx(self, score):
        score = np.float32(score)
        if np.isnan(score):
            return self.T // 2
        lo, hi = 0, self.T                                                       # bisect (:23-30)
        while lo < hi:
            mid = (lo + hi) // 2
            if self.thr[mid] < score:
                lo = mid + 1
            else:
                hi = mid
        return lo

    def precision(self, i):
        return {k: 1.0 if self.s["fp"][k][i] == 0 else float(np.float32(self.s["tp"][k][i]) / np.float32(self.s["tp"][k][i] + self.s["fp"][k][i]))
                for k in self.classes}

    def recall(self, i):
        return {k: 1.0 if self.s["fn"][k][i] == 0 else float(np.float32(self.s["tp"][k][i]) / np.float32(self.s["tp"][k][i] + self.s["fn"][k][i]))
                for k in self.classes}

    def ap(self):
        p = [self.precision(i) for i in range(self.T)]
        r = [self.recall(i) for i in range(self.T)]
        return {k: float(-np.trapezoid([x[k] for x in p], [x[k] for x in r])) for k in self.classes}

    def mota(self, i):
        s = self.s
        return {k: 1 - float(s["fp"][k][i] + s["fn"][k][i] + s["id_switches"][k][i]) / s["ngt"][k] for k in self.classes}

    def frame_ratio(self, i, thr, high):
        thr = np.float32(thr)
        out = {}
        for k in self.classes:
            v = 0
            for tid, c in self.s["ngt_tracked"][k][i].items():
                ratio = np.float32(float(c) / self.s["ngt_ids"][k][tid])
                v += int(ratio > thr) if high else int(ratio < thr)
            out[k] = float(v) / len(self.s["ngt_ids"][k])
        return out
