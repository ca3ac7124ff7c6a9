"""d3d_amd.benchmarks -- DetectionEvaluator.calc_stats of the reference (d3d/benchmarks.pyx:60-300) on arrays.

Boxes are [n,9] float32 rows (label, score, x, y, z, lx, ly, lz, yaw) -- Target3DArray.to_numpy's layout
(d3d/abstraction.pyx:263-272); the container classes of d3d.abstraction and the dataset-specific class enums are outside
this library's scope, classes are plain integers here.  The pairwise distance matrix (d3d_match_distance) and the
score-ordered association (d3d_score_match) run on the GPU; the per-threshold counts and means over the n + m matched indices
are numpy.  Two associations:
* the default, `reference_compat=True`: the reference's own, result for result -- one association PER score threshold
  (benchmarks.pyx:218-238) with ScoreMatcher.match's literal pairing of the two orders (matcher.pyx:142-162,
  d3d_amd.tracking.matcher.score_match_reference_compat);
* `reference_compat=False`: every detection walks its own nearest ground truths -- then ONE association serves all thresholds
  (a box's choice only depends on the boxes of higher score), 40 times less work.  Equal to the first wherever no detection
  has two acceptable ground truths.

SegmentationEvaluator / SegmentationStats are the reference's (benchmarks.pyx:891-1213): the per-point counting of calc_stats
(collect_labels / collect_labels_pano, :977-1075) is d3d_segeval on the GPU, the bookkeeping over at most 255 classes is host
arithmetic as the reference does it.

TrackingEvaluator / TrackingEvalStats are the reference's (benchmarks.pyx:449-890): a frame's carry-over, association and
id-switch / fragment counting is d3d_match_distance + d3d_track_frame on the GPU with the carried assignments kept on the
device; the per-frame tid maps and the metrics are host arithmetic.  DetectionEvaluator also has the reference's accumulation
and metrics (reset, add_stats, get_stats, tp .. ap, acc_*, summary; :146-447).
"""
import ctypes
import math
from enum import Enum

import numpy as np
import torch

from . import _lib
from ._rows import device_of
from .tracking.matcher import DistanceTypes, ReferenceAssociation, prepare_boxes, score_match
from .utils import Dict


class DetectionEvaluator:
    """Benchmark for object detection; targets association is done by score sorting (benchmarks.pyx:84-149).

    Extension beyond the reference: calc_stats_batch evaluates many stacked frames in one call."""

    def __init__(self, classes, min_overlaps, pr_sample_count=40, min_score=0, pr_sample_scale="log10", reference_compat=True):
        self.reference_compat = bool(reference_compat)
        classes = list(classes) if isinstance(classes, (list, tuple)) else [classes]
        assert len(classes) > 0
        self._class_type = type(classes[0]) if isinstance(classes[0], Enum) else None                 # :105-112
        values = [int(getattr(c, "value", c)) for c in classes]
        self._classes = list(dict.fromkeys(values))                                                  # (an unordered_set)
        if isinstance(min_overlaps, (list, tuple)):
            self._max_distance = {c: 1 - v for c, v in zip(values, min_overlaps)}                    # :114-115
        elif isinstance(min_overlaps, (int, float)):
            self._max_distance = {c: 1 - min_overlaps for c in self._classes}
        else:
            raise ValueError("min_overlaps should be a list or a single value")
        self._pr_nsamples = int(pr_sample_count)
        self._min_score = float(min_score)
        if pr_sample_scale == "lin":                                                                 # :125-134
            thresholds = np.linspace(min_score, 1, pr_sample_count, endpoint=False, dtype=np.float32)
        elif pr_sample_scale.startswith("log"):
            logstart, logend = 1, int(pr_sample_scale[3:] or "10")
            thresholds = np.geomspace(logstart, logend, pr_sample_count + 1, dtype=np.float32)
            thresholds = (thresholds - logstart) * (1 - min_score) / (logend - logstart)
            thresholds = (1 - thresholds)[:0:-1]
        else:
            raise ValueError("Unrecognized PR sample type")
        self._pr_thresholds = np.asarray(thresholds, dtype=np.float32)
        self._stats = self._new_stats()

    def _new_stats(self):
        """DetectionEvalStats.initialize (:66-78): counts 0, accuracies NaN"""
        T = self._pr_nsamples
        st = Dict(ngt={c: 0 for c in self._classes})
        for k in _COUNT_FIELDS:
            st[k] = {c: [0] * T for c in self._classes}
        for k in ("acc_angular", "acc_box", "acc_iou", "acc_dist", "acc_var"):    # _ACC_FIELDS in the order get_stats() lists them
            st[k] = {c: [math.nan] * T for c in self._classes}
        return st

    @property
    def score_thresholds(self):
        return self._pr_thresholds

    def reset(self):
        self._stats = self._new_stats()

    def add_stats(self, stats):
        """Add statistics from calc_stats into database (:300-327): counts summed, the accuracies merged by fp32 wmean
        (math/__init__.pxd:4-9) weighted by the true positives"""
        T = self._pr_nsamples
        for k in self._classes:
            self._stats.ngt[k] += stats.ngt[k]
            otp, ntp = np.asarray(self._stats.tp[k], np.int64), np.asarray(stats.tp[k], np.int64)
            for name in _ACC_FIELDS:
                mine = getattr(self._stats, name)
                mine[k] = _wmean(mine[k], otp, getattr(stats, name)[k], ntp)
            for name in _COUNT_FIELDS:
                mine, theirs = getattr(self._stats, name), getattr(stats, name)[k]
                mine[k] = [int(mine[k][i]) + int(theirs[i]) for i in range(T)]

    def get_stats(self):
        """Summarize current state of the benchmark counters"""
        return self._stats

    def _get_score_idx(self, score):
        """:321-325: NaN -> the middle threshold, otherwise bisect_left over the (fp32) thresholds"""
        score = np.float32(score)
        if np.isnan(score):
            return self._pr_nsamples // 2
        return int(np.searchsorted(self._pr_thresholds, score, side="left"))

    def _key(self, k):
        return k if self._class_type is None else self._class_type(k)

    def _name(self, k):
        return str(k) if self._class_type is None else self._class_type(k).name

    def _at(self, table, score):
        i = self._get_score_idx(score)
        return {self._key(k): table[k][i] for k in self._classes}

    def gt_count(self):
        return {self._key(k): self._stats.ngt[k] for k in self._classes}

    def dt_count(self, score=math.nan):
        return self._at(self._stats.ndt, score)

    def tp(self, score=math.nan):
        """Return true positive count. If score is not specified, return the median value"""
        return self._at(self._stats.tp, score)

    def fp(self, score=math.nan):
        """Return false positive count. If score is not specified, return the median value"""
        return self._at(self._stats.fp, score)

    def fn(self, score=math.nan):
        """Return false negative count. If score is not specified, return the median value"""
        return self._at(self._stats.fn, score)

    def _per_class(self, fn, score, return_all):
        """fn(k, i) for every class at one threshold, or (return_all) for every threshold"""
        if return_all:
            return {self._key(k): [fn(k, i) for i in range(self._pr_nsamples)] for k in self._classes}
        i = self._get_score_idx(score)
        return {self._key(k): fn(k, i) for k in self._classes}

    def precision(self, score=math.nan, return_all=False):
        s = self._stats
        return self._per_class(lambda k, i: _calc_precision(s.tp[k][i], s.fp[k][i]), score, return_all)

    def recall(self, score=math.nan, return_all=False):
        s = self._stats
        return self._per_class(lambda k, i: _calc_recall(s.tp[k][i], s.fn[k][i]), score, return_all)

    def fscore(self, score=math.nan, beta=1, return_all=False):
        s, b2 = self._stats, np.float32(beta) * np.float32(beta)
        return self._per_class(lambda k, i: _calc_fscore(s.tp[k][i], s.fp[k][i], s.fn[k][i], b2), score, return_all)

    def ap(self):
        """Calculate (mean) average precision (:390-397); the curve runs from bottom right to top left, hence the sign"""
        p, r = self.precision(return_all=True), self.recall(return_all=True)
        return {k: float(-np.trapezoid(p[k], r[k])) for k in p}

    def acc_iou(self, score=math.nan):
        return self._at(self._stats.acc_iou, score)

    def acc_box(self, score=math.nan):
        return self._at(self._stats.acc_box, score)

    def acc_dist(self, score=math.nan):
        return self._at(self._stats.acc_dist, score)

    def acc_angular(self, score=math.nan):
        return self._at(self._stats.acc_angular, score)

    def _summary_accuracy(self, lines, k, score_thres, score_idx):
        s = self._stats
        lines.append("\tMean IoU (score > %.2f):\t\t%.3f" % (score_thres, s.acc_iou[k][score_idx]))
        lines.append("\tMean angular error (score > %.2f):\t%.3f" % (score_thres, s.acc_angular[k][score_idx]))
        lines.append("\tMean distance (score > %.2f):\t\t%.3f" % (score_thres, s.acc_dist[k][score_idx]))
        lines.append("\tMean box error (score > %.2f):\t\t%.3f" % (score_thres, s.acc_box[k][score_idx]))
        if not math.isinf(s.acc_var[k][score_idx]):
            lines.append("\tMean variance error (score > %.2f):\t%.3f" % (score_thres, s.acc_var[k][score_idx]))

    def summary(self, score_thres=0.8, verbose=False):
        """Print default summary (into returned string) (:410-447); int classes print as the int"""
        score_thres = _f32(score_thres)
        score_idx = self._get_score_idx(score_thres)
        lines = [""]
        precision, recall = self.precision(score_thres), self.recall(score_thres)
        fscore, ap = self.fscore(return_all=True), self.ap()
        lines.append("========== Benchmark Summary ==========")
        for k in self._classes:
            typed_k = self._key(k)
            if verbose:
                lines.append("Results for %s:" % self._name(k))
                lines.append("\tTotal processed targets:\t%d gt boxes, %d dt boxes" % (
                    self._stats.ngt[k], max(self._stats.ndt[k])))
                lines.append("\tPrecision (score > %.2f):\t%.3f" % (score_thres, precision[typed_k]))
                lines.append("\tRecall (score > %.2f):\t\t%.3f" % (score_thres, recall[typed_k]))
                lines.append("\tMax F1:\t\t\t\t%.3f" % max(fscore[typed_k]))
                lines.append("\tAP:\t\t\t\t%.3f" % ap[typed_k])
                lines.append("")
                self._summary_accuracy(lines, k, score_thres, score_idx)
            else:
                lines.append("\tResults for %s: AP=%.3f" % (self._name(k), ap[typed_k]))
        lines.append("mAP: %.3f" % np.mean(list(ap.values())))
        lines.append("========== Summary End ==========")
        return "\n".join(lines)

    def calc_stats(self, gt_boxes, dt_boxes):
        """-> Dict(ngt{c}, ndt{c}[T], tp, fp, fn, acc_iou{c}[T], acc_angular, acc_dist, acc_box, acc_var) as
        DetectionEvalStats (benchmarks.pyx:60-82, 178-283); both box sets must be in the same frame"""
        gt = np.ascontiguousarray(gt_boxes, dtype=np.float32).reshape(-1, 9)
        dt = np.ascontiguousarray(dt_boxes, dtype=np.float32).reshape(-1, 9)
        gt_tag, dt_tag = gt[:, 0].astype(np.int64), dt[:, 0].astype(np.int64)
        dt_score = dt[:, 1]
        if self.reference_compat:
            return self._calc_stats_per_threshold(gt, dt)
        if len(gt) and len(dt):
            cache = prepare_boxes(dt, gt, DistanceTypes.RIoU)                                        # :188-189
            sm, dm = score_match(cache, dt_score, dt_tag, gt_tag, self._max_distance)
            dm = dm.cpu().numpy().astype(np.int64)
            sm = sm.cpu().numpy().astype(np.int64)
            matched = dm >= 0
            iou = np.zeros((len(gt),), np.float32)
            iou[matched] = (1 - cache[dm[matched], np.nonzero(matched)[0]]).cpu().numpy()            # :243
        else:
            sm, dm = np.full((len(dt),), -1, np.int64), np.full((len(gt),), -1, np.int64)
            iou = np.zeros((len(gt),), np.float32)
        return self._stats_of_match(gt, dt, sm, dm, iou)

    def _stats_of_match(self, gt, dt, sm, dm, iou):
        """the stats of a frame from ONE association (reference_compat=False): sm[n] / dm[m] int64 partners or -1, iou[m] fp32
        = 1 - distance of a ground truth's pair, 0 without one.  calc_stats and calc_stats_batch share it."""
        classes, thr = self._classes, self._pr_thresholds
        gt_tag, dt_tag = gt[:, 0].astype(np.int64), dt[:, 0].astype(np.int64)
        dt_score = dt[:, 1]
        out = Dict((k, {}) for k in ("ngt",) + _COUNT_FIELDS + _ACC_FIELDS)
        matched = dm >= 0
        partner = np.where(matched, dm, 0)
        # a ground-truth box is a true positive at threshold t iff its detection is selected there (score >= t)  (:220-238)
        gscore = np.where(matched, dt_score[partner] if len(dt) else 0.0, -np.inf)
        dmatched = sm >= 0
        vals = np.stack(_pair_terms(gt, dt[partner], iou)).astype(np.float64) if len(dt) else np.zeros((4, len(gt)))   # [4, m]

        def at_least(scores):
            """#(scores >= t) for every threshold t: one sort instead of a [len, T] comparison (:224-225: `score < thres` is
            skipped, so a NaN score is selected at EVERY threshold there -- counted apart, np.sort files NaNs last)"""
            nan = int(np.isnan(scores).sum())
            srt = np.sort(scores[~np.isnan(scores)])
            return (len(srt) - np.searchsorted(srt, thr, side="left") + nan).astype(np.int64)
        for c in classes:
            g, d = gt_tag == c, dt_tag == c
            out.ngt[c] = int(g.sum())
            out.ndt[c] = at_least(dt_score[d]).tolist()
            out.fp[c] = at_least(dt_score[d & ~dmatched]).tolist()
            # the true positives of threshold t are the matched boxes with gscore >= t: sorted by that score, every threshold is
            # a prefix -- counts by searchsorted, the sums of the accuracy terms by one cumulative sum (float64, rounded once)
            gs = gscore[g]
            o = np.argsort(-gs, kind="stable")
            gs_sorted = gs[o]
            tp = np.searchsorted(-gs_sorted, -thr, side="right").astype(np.int64)                      # #(gscore >= t)
            out.tp[c] = tp.tolist()
            out.fn[c] = (out.ngt[c] - tp).tolist()
            csum = np.concatenate([np.zeros((4, 1)), np.cumsum(vals[:, g][:, o], axis=1)], axis=1)      # [4, mc + 1]
            with np.errstate(invalid="ignore", divide="ignore"):
                means = np.where(tp[None, :] > 0, csum[:, tp] / tp[None, :], np.nan).astype(np.float32)
            for name, v in zip(_ACC_FIELDS, list(means) + [_acc_var(tp)]):
                out[name][c] = v.tolist()
        return out

    def _calc_stats_per_threshold(self, gt, dt):
        """benchmarks.pyx:188-283 as written: select the detections of a threshold, associate (the literal pairing), count"""
        T, C, thr = self._pr_nsamples, len(self._classes), self._pr_thresholds
        gt_tag, dt_tag = gt[:, 0].astype(np.int64), dt[:, 0].astype(np.int64)
        gslot, dslot = _class_slots(self._classes, gt), _class_slots(self._classes, dt)
        dt_score = dt[:, 1]
        gt_idx = np.nonzero(gslot >= 0)[0]                                                            # :205-212
        cache = prepare_boxes(dt, gt, DistanceTypes.RIoU) if len(gt) and len(dt) else None             # :188-189
        # the 40 associations share what does not depend on the threshold (the ground truths' columns of the cache, which pairs are
        # acceptable) and go to the device as batched calls (ReferenceAssociation.match_many: one for a frame, a few for config 4's
        # 20 k x 5 k), nothing read back in between; the results are fetched together
        assoc = gt_idx_t = None
        if cache is not None and len(gt_idx):
            assoc = ReferenceAssociation(cache, dt_score, dt_tag, gt_tag, self._max_distance, gt_idx)
            gt_idx_t = torch.from_numpy(gt_idx).to(cache.device)
        sel = (dslot >= 0)[None, :] & ~(dt_score[None, :] < thr[:, None])                            # [T, n]: :219-228 (`score < thres`: skip)
        dt_idxs = [np.nonzero(sel[t])[0] for t in range(T)]
        md = len(gt_idx)
        sm_all = np.full((T, len(dt)), -1, np.int32)
        dm_g = np.full((T, md), -1, np.int32)                                                       # dst_match over the ground truths taking part
        iou_all = np.zeros((T, md), np.float32)
        if assoc is not None:
            sm_t, dm_t = assoc.match_many(dt_idxs)                                                     # :231-232, all thresholds
            dmg_t = dm_t.index_select(1, gt_idx_t)
            iou_t = 1 - cache[dmg_t.long().clamp_min(0), gt_idx_t[None, :]]                            # :243 (entries of the unmatched: unused)
            sm_all, dm_g, iou_all = sm_t.cpu().numpy(), dmg_t.cpu().numpy(), iou_t.cpu().numpy()
        # the counts and means of :236-283 for all thresholds at once: the K matched (threshold, ground truth) pairs as flat arrays
        tt, jj = np.nonzero(dm_g >= 0)
        gi = gt_idx[jj]
        tp, acc = _bin_means(gslot[gi].astype(np.int64) * T + tt, (C, T), _pair_terms(gt[gi], dt[dm_g[tt, jj]], iou_all[tt, jj]))
        ngt = np.bincount(gslot[gt_idx], minlength=C)
        ndt, fp = np.zeros((C, T), np.int64), np.zeros((C, T), np.int64)
        unmatched = sm_all < 0
        for i in range(C):
            dc = sel & (dslot == i)[None, :]
            ndt[i], fp[i] = dc.sum(1), (dc & unmatched).sum(1)                                         # :262-265
        return self._frame_dicts(ngt[None], [a[None] for a in [ndt, tp, fp, ngt[:, None] - tp] + acc])[0]   # (fn: :236-240)

    # ------------------------------------------------------------------ many frames per call
    def calc_stats_batch(self, gt_boxes, dt_boxes, gt_frame_offsets, dt_frame_offsets):
        """Extension (not in the reference): F frames stacked, frame f = gt rows gt_frame_offsets[f] .. gt_frame_offsets[f + 1]
        and dt rows dt_frame_offsets[f] .. dt_frame_offsets[f + 1] (F + 1 offsets each, rising from 0 to the number of rows;
        numpy arrays or tensors on any device).  -> list of F stats, element f exactly what calc_stats(gt_f, dt_f) returns
        (the same keys, types and counts, the float fields bit for bit), in both settings of reference_compat; nothing is added
        to the totals (add_stats does).  The frames go to the device in chunks of at most _DET_MAX_FRAMES frames and
        _DET_MAX_CACHE_BYTES of distance cache, two launches each (d3d_deteval_batched), with one upload before and one fetch
        after all of them.  Three kinds of frame go through calc_stats one by one instead: those with more boxes on a side than
        d3d_deteval_frame_max(); with reference_compat, those whose selected in-class scores hold a NaN or a tie (calc_stats
        orders every threshold's selection with numpy's unstable argsort, which only a run on the same subset reproduces);
        and every frame when the score thresholds do not rise."""
        gt, dt = _host_rows(gt_boxes, np.float32, 9), _host_rows(dt_boxes, np.float32, 9)
        go, do = _frame_offsets("frame offsets must rise from 0 to the number of boxes",
                                (gt_frame_offsets, len(gt)), (dt_frame_offsets, len(dt)))
        F = len(go) - 1
        if F == 0:
            return []
        h = self._batch_prepare(gt, dt, go, do)
        stats = [None] * F
        fallback = h["fallback"]
        good = np.nonzero(~fallback)[0]
        if len(good) < F:                                  # the rows of the frames that stay, stacked anew
            gsel, dsel = np.repeat(~fallback, np.diff(go)), np.repeat(~fallback, np.diff(do))
            go2, do2 = np.zeros((len(good) + 1,), np.int64), np.zeros((len(good) + 1,), np.int64)
            np.cumsum(np.diff(go)[good], out=go2[1:])
            np.cumsum(np.diff(do)[good], out=do2[1:])
            h = self._batch_prepare(gt[gsel], dt[dsel], go2, do2) if len(good) else None
        pending = self._batch_launch(h, device_of(gt_boxes, dt_boxes)) if len(good) else None
        for f in np.nonzero(fallback)[0]:
            stats[f] = self.calc_stats(gt[go[f]:go[f + 1]], dt[do[f]:do[f + 1]])
        if pending is not None:
            for f, st in zip(good, self._batch_stats(h, pending.cpu().numpy())):
                stats[f] = st
        return stats

    def _batch_prepare(self, gt, dt, go, do):
        """what the host knows of the stacked frames before the device runs, as flat arrays: class slots, every frame's in-class
        detections from the best score down (NaN first, ties in index order: torch.sort(descending, stable) as score_match
        calls it, of which every threshold's selection is a prefix), the selected counts, and which frames fall back"""
        T, C, thr = self._pr_nsamples, len(self._classes), self._pr_thresholds
        F = len(go) - 1
        nf, mf = np.diff(do), np.diff(go)
        fd, fg = np.repeat(np.arange(F), nf), np.repeat(np.arange(F), mf)
        gslot, dslot = _class_slots(self._classes, gt), _class_slots(self._classes, dt)
        score = dt[:, 1]
        nan, inc = np.isnan(score), dslot >= 0
        order = np.lexsort((np.where(nan, np.float32(0), -score), ~nan, ~inc, fd))
        base = np.repeat(do[:-1], nf)
        perm = (order - base).astype(np.int32)
        rank = np.empty((len(dt),), np.int32)
        rank[order] = np.arange(len(dt)) - base
        rank[~inc] = -1
        # a detection is selected at the thresholds t < sel_upto: `score < thres` skips (:224-225), so a NaN score never does
        rising = bool(np.all(np.diff(thr) >= 0))
        sel_upto = np.where(nan, T, np.searchsorted(thr, score, side="right")) if rising else np.full((len(dt),), T)
        hist = np.bincount(((fd * C + dslot) * (T + 1) + sel_upto)[inc], minlength=F * C * (T + 1)).reshape(F, C, T + 1)
        ndt = np.cumsum(hist[:, :, ::-1], axis=2)[:, :, ::-1][:, :, 1:]                                # [F, C, T]: #(sel_upto > t)
        ngt = np.bincount((fg * C + gslot)[gslot >= 0], minlength=F * C).reshape(F, C)
        bound = _lib.load().d3d_deteval_frame_max()
        fallback = (nf > bound) | (mf > bound)
        if self.reference_compat:
            if not rising:
                fallback[:] = True
            fallback[fd[nan & inc]] = True
            so, fo, io, uo = score[order], fd[order], inc[order], sel_upto[order]
            tie = (fo[1:] == fo[:-1]) & io[1:] & io[:-1] & (so[1:] == so[:-1]) & (uo[1:] > 0)
            fallback[fo[1:][tie]] = True
        return dict(gt=gt, dt=dt, go=go, do=do, nf=nf, mf=mf, gslot=gslot, dslot=dslot, perm=perm, rank=rank, ndt=ndt, ngt=ngt,
                    fallback=fallback)

    def _batch_launch(self, h, dev):
        """one upload, d3d_deteval_batched per chunk of frames, no wait -> the device tensor of all chunks' results: int32
        [gt_match | gt_iou] over the problems' ground truths, then (reference_compat=False) dt_match over the detections"""
        lib = _lib.load()
        T, C, literal = self._pr_nsamples, len(self._classes), self.reference_compat
        go, do, nf, mf = h["go"], h["do"], h["nf"], h["mf"]
        F, N, M = len(nf), len(h["dt"]), len(h["gt"])
        P = T if literal else 1
        # the distance thresholds: a class without one reads 0.0 in the literal association (unordered_map::operator[],
        # matcher.pyx:112) and takes no part in the other (score_match)
        maxd = np.array([self._max_distance.get(c, 0.0 if literal else np.nan) for c in self._classes], np.float32)
        # the slots of a problem: the detections selected at its threshold; every in-class detection of its frame
        slots = h["ndt"].sum(1).astype(np.int32) if literal else \
            np.bincount(np.repeat(np.arange(F), nf)[h["dslot"] >= 0], minlength=F).astype(np.int32)
        pairs = nf * mf
        chunks, f0 = [], 0
        while f0 < F:                                      # as many frames as the caps allow, one at least
            f1, nbytes = f0, 0
            while f1 < F and (f1 == f0 or (f1 - f0 < _DET_MAX_FRAMES and nbytes + 4 * pairs[f1] <= _DET_MAX_CACHE_BYTES)):
                nbytes += 4 * int(pairs[f1])
                f1 += 1
            chunks.append((f0, f1))
            f0 = f1
        shared = {k: h[k] for k in ("dt", "gt", "dslot", "gslot", "perm", "rank")}
        shared.update(slots=slots, maxd=maxd)
        offs = []                                          # a chunk's offsets: detection rows, ground-truth rows, cache entries
        for f0, f1 in chunks:
            co = np.zeros((f1 - f0 + 1,), np.int64)
            np.cumsum(pairs[f0:f1], out=co[1:])
            offs += [do[f0:f1 + 1] - do[f0], go[f0:f1 + 1] - go[f0], co]
        npairs = [int(co[-1]) for co in offs[2::3]]
        with torch.cuda.device(dev):
            blob, addr = _upload(dev, list(shared.values()) + offs)
            at, chunk_at = dict(zip(shared, addr)), addr[len(shared):]
            out = torch.empty((max(2 * P * M + (0 if literal else N), 1),), dtype=torch.int32, device=dev)
            obase, stream = out.data_ptr(), _lib.stream_ptr()
            ws = _lib.workspace(max(lib.d3d_deteval_batched_workspace_bytes(k, 0) for k in npairs), dev)
            for i, (f0, f1) in enumerate(chunks):
                d0, g0 = int(do[f0]), int(go[f0])
                dof, gof, cof = chunk_at[3 * i:3 * i + 3]
                rc = lib.d3d_deteval_batched(
                    ctypes.c_void_p(at["dt"] + 36 * d0), ctypes.c_void_p(at["gt"] + 36 * g0), ctypes.c_void_p(dof),
                    ctypes.c_void_p(gof), ctypes.c_void_p(cof), f1 - f0, npairs[i], int(nf[f0:f1].max()), int(mf[f0:f1].max()),
                    ctypes.c_void_p(at["dslot"] + 4 * d0), ctypes.c_void_p(at["gslot"] + 4 * g0),
                    ctypes.c_void_p(at["perm"] + 4 * d0), ctypes.c_void_p(at["rank"] + 4 * d0),
                    ctypes.c_void_p(at["slots"] + 4 * P * f0), T, ctypes.c_void_p(at["maxd"]), C, 1 if literal else 0,
                    None, ctypes.c_void_p(obase + 4 * P * g0), ctypes.c_void_p(obase + 4 * (P * M + P * g0)),
                    None if literal else ctypes.c_void_p(obase + 4 * (2 * M + d0)), _lib.ptr(ws), ws.numel(), stream)
                _lib.check(rc, "deteval_batched")
        return out

    def _batch_stats(self, h, res):
        """the frames' stats from the fetched results (_batch_launch's layout)"""
        T, C = self._pr_nsamples, len(self._classes)
        gt, dt, go, do, mf = h["gt"], h["dt"], h["go"], h["do"], h["mf"]
        F, N, M = len(mf), len(dt), len(gt)
        if not self.reference_compat:                      # one association per frame: calc_stats' own epilogue, frame by frame
            dm, iou, sm = res[:M].astype(np.int64), res[M:2 * M].view(np.float32), res[2 * M:2 * M + N].astype(np.int64)
            return [self._stats_of_match(gt[go[f]:go[f + 1]], dt[do[f]:do[f + 1]], sm[do[f]:do[f + 1]], dm[go[f]:go[f + 1]],
                                         iou[go[f]:go[f + 1]]) for f in range(F)]
        # the K matched (frame, threshold, ground truth) triples in that order, binned by (frame, class, threshold): a bin receives
        # its terms in ascending ground-truth order, as calc_stats' bins of one frame do, so the sums have the same bits
        gm, iou = res[:T * M], res[T * M:2 * T * M].view(np.float32)
        e = np.nonzero(gm >= 0)[0]
        fe = np.searchsorted(T * go[1:], e, side="right")             # frame f's [T, m_f] block starts at T * go[f]
        rem = e - T * go[fe]
        te = rem // np.maximum(mf[fe], 1)
        gi, di = go[fe] + (rem - te * mf[fe]), do[fe] + gm[e]
        tp, acc = _bin_means((fe * C + h["gslot"][gi]) * T + te, (F, C, T), _pair_terms(gt[gi], dt[di], iou[e]))
        ndt, ngt = h["ndt"], h["ngt"]
        return self._frame_dicts(ngt, [ndt, tp, ndt - tp, ngt[:, :, None] - tp] + acc)

    def _frame_dicts(self, ngt, cols):
        """ngt [F, C] and the arrays [F, C, T] of _COUNT_FIELDS + _ACC_FIELDS, in that order -> the F frames' stats"""
        ngt, cols = ngt.tolist(), [col.tolist() for col in cols]
        stats = []
        for f in range(len(ngt)):
            st = Dict(ngt=dict(zip(self._classes, ngt[f])))
            for name, col in zip(_COUNT_FIELDS + _ACC_FIELDS, cols):
                st[name] = dict(zip(self._classes, col[f]))
            stats.append(st)
        return stats


_DET_MAX_FRAMES = 16384                # frames of one d3d_deteval_batched call (one wavefront per frame and threshold: 40
                                       # thresholds make 655 k workgroups, seconds of evaluator input to prepare and fetch at once)
_DET_MAX_CACHE_BYTES = 256 << 20       # and the bytes of its ragged distance cache, which lives in the workspace arena
# the fields of a frame's stats beside ngt, in the order calc_stats lists them: counts and accuracies per class and threshold
_COUNT_FIELDS = ("ndt", "tp", "fp", "fn")
_ACC_FIELDS = ("acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var")


def _class_slots(classes, boxes):
    """the position in `classes` of the class of every box [n, 9] (int32), -1 for a class that is not among them"""
    tags, values = boxes[:, 0].astype(np.int64), np.asarray(classes, np.int64)
    by_value = np.argsort(values, kind="stable")
    at = np.minimum(np.searchsorted(values[by_value], tags), len(values) - 1)
    return np.where(values[by_value[at]] == tags, by_value[at], -1).astype(np.int32)


def _pair_terms(ga, da, iou):
    """the accuracy terms of K matched pairs (benchmarks.pyx:252-257, 648-653) from the ground truths' rows ga [K, 9], their detections'
    rows da [K, 9] and the pairs' IoUs -> fp32 [K] each, in _ACC_FIELDS' order: the IoU, the angular error (quatdiff of two yaw
    rotations / pi), the distance of the centres and of the box sizes (np.linalg.norm(., axis=1) spelled out --
    sqrt(add.reduce(x * x)) over three terms, the same bits)"""
    dp, db = ga[:, 2:5] - da[:, 2:5], ga[:, 5:8] - da[:, 5:8]
    dyaw = ga[:, 8] - da[:, 8]
    return (iou, np.abs((dyaw + np.pi) % (2 * np.pi) - np.pi) / np.pi,
            np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2]),
            np.sqrt((db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1]) + db[:, 2] * db[:, 2]))


def _acc_var(tp):
    """no variances travel in the [n,9] arrays: orientation_var = 0 -> -inf per match (:259-267, 655-663), NaN without one"""
    return np.where(tp > 0, -np.inf, np.nan)


def _bin_means(key, shape, terms):
    """the counts and means of benchmarks.pyx:150-174, 236-283 over bins (of frame, class and threshold): key[K] = the bin of every
    matched pair, `shape` = the bins' (their number is its product), terms = _pair_terms' arrays [K] -> tp (int64) and the
    arrays of _ACC_FIELDS, all of `shape`.  A mean is the float32 terms summed in float64 in the order of the pairs, one
    division, one rounding to float32; NaN for a bin without a pair."""
    nbins = math.prod(shape)
    tp = np.bincount(key, minlength=nbins)
    acc = []
    for v in terms:
        ssum = np.bincount(key, weights=v.astype(np.float64), minlength=nbins)
        with np.errstate(invalid="ignore", divide="ignore"):
            acc.append(np.where(tp > 0, (ssum / tp).astype(np.float32), np.float32(np.nan)).reshape(shape))
    return tp.reshape(shape), acc + [_acc_var(tp).reshape(shape)]


def _frame_offsets(message, *sides):
    """the frame offsets of stacked rows, checked -> one int64 array per side = (offsets, number of rows): F + 1 offsets that rise
    from 0 to the number of rows (ValueError(message) otherwise), every side describing the same frames"""
    offs = [_host_rows(offsets, np.int64, 0) for offsets, _ in sides]
    for off, (_, n) in zip(offs, sides):
        if len(off) < 1 or off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 0):
            raise ValueError(message)
    if any(len(off) != len(offs[0]) for off in offs):
        raise ValueError("gt_frame_offsets and dt_frame_offsets must describe the same frames")
    return offs


def _upload(dev, arrays):
    """host arrays to the GPU `dev` in ONE copy -> (the device buffer, the device address of every array in it); every array
    starts at a multiple of 256 bytes of the buffer.  _lib.ship's job for callers that step through the rows by bytes (a
    chunk's first frame, `+ 36 * d0`), send uint64 ids and hand the C entry points an address for every array, an empty one
    included; the caller holds the buffer until its launches are queued"""
    parts, starts, pos = [], [], 0
    for a in arrays:
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        starts.append(pos)
        parts.append(b)
        pad = _aligned(len(b)) - len(b)
        if pad:
            parts.append(np.zeros((pad,), np.uint8))
        pos += len(b) + pad
    blob = torch.from_numpy(np.concatenate(parts)).to(dev)
    return blob, [blob.data_ptr() + s for s in starts]


def _wmean(a, wa, b, wb):
    """math/__init__.pxd:4-9 elementwise, in fp32: a if wb == 0, b if wa == 0, (a * wa + b * wb) / (wa + wb) otherwise"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mixed = (a * wa.astype(np.float32) + b * wb.astype(np.float32)) / (wa + wb).astype(np.float32)
    return np.where(wa == 0, b, np.where(wb == 0, a, mixed)).astype(np.float32).tolist()


def _calc_precision(tp, fp):                    # :32-34 (fp32)
    return 1.0 if fp == 0 else _f32(np.float32(tp) / np.float32(tp + fp))


def _calc_recall(tp, fn):                       # :35-37 (fp32)
    return 1.0 if fn == 0 else _f32(np.float32(tp) / np.float32(tp + fn))


def _calc_fscore(tp, fp, fn, b2):               # :38-39 (fp32; 0 / 0 is NaN under cdivision)
    one = np.float32(1) + b2
    with np.errstate(invalid="ignore", divide="ignore"):
        return _f32(one * np.float32(tp) / (one * np.float32(tp) + b2 * np.float32(fn) + np.float32(fp)))


_SEG_FIELDS = ("tp", "fp", "fn", "itp", "ifp", "ifn", "cumiou")
_SEG_MAX_FRAMES = 65535                # frames of one d3d_segeval call (the frame index is 16 bits of the pair key)


class SegmentationStats:
    """Counts of one frame (or of many, summed) per class (benchmarks.pyx:891-929): tp / fp / fn of semantic segmentation
    (points), itp / ifp / ifn of panoptic segmentation (segments), cumiou = the sum of the IoUs of the matched segments
    (fp32, as the reference keeps it).  Plain dicts class -> value; pickles (the reference auto-pickles, :891)."""

    def __init__(self):
        for k in _SEG_FIELDS:
            setattr(self, k, {})

    def initialize(self, classes):
        """every counter of every class to 0 (:916-924)"""
        for k in _SEG_FIELDS:
            setattr(self, k, {c: (0.0 if k == "cumiou" else 0) for c in classes})

    def as_object(self):
        return dict(tp=dict(self.tp), fp=dict(self.fp), fn=dict(self.fn),
                    itp=dict(self.itp), ifp=dict(self.ifp), ifn=dict(self.ifn), cumiou=dict(self.cumiou))

    def __eq__(self, other):
        return isinstance(other, SegmentationStats) and self.as_object() == other.as_object()

    def __repr__(self):
        return "SegmentationStats(%r)" % (self.as_object(),)


def _f32(x):
    return float(np.float32(x))


def _is_u16(x):
    return x.dtype == torch.uint16 if torch.is_tensor(x) else np.asarray(x).dtype == np.uint16


def _seg_array(x, dtype, tdtype, dev, what):
    """a contiguous 1-D device tensor of x (numpy array or torch tensor) without changing its values"""
    if torch.is_tensor(x):
        if x.dtype != tdtype:
            raise ValueError("%s: expected %s, got %s" % (what, tdtype, x.dtype))
        x = x.reshape(-1)
        if x.device != dev:
            x = x.to(dev)
        return x.contiguous()
    x = np.asarray(x)
    if x.dtype != dtype:
        raise ValueError("%s: expected %s, got %s" % (what, np.dtype(dtype).name, x.dtype))
    return torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to(dev)


class SegmentationEvaluator:
    """Benchmark for semantic and panoptic segmentation (benchmarks.pyx:933-1213; cityscapesScripts' panoptic evaluation).

    Extension beyond the reference: calc_stats_batch counts many stacked frames in one device call."""

    def __init__(self, classes, background=0, min_points=0):
        """
        :param classes: classes to be considered during evaluation, other classes are all considered as background
        :param background: class to be considered as background class
        :param min_points: minimum number of points when calculating segments in panoptic evaluation
        """
        if not isinstance(classes, (list, tuple)):                                                   # :950-963
            classes = [classes]
        assert len(classes) > 0
        if isinstance(classes[0], Enum):
            self._class_type = type(classes[0])
            values = set(c.value for c in classes)
        elif isinstance(classes[0], int):
            self._class_type = None
            values = set(classes)
        else:
            raise ValueError("Classes should be int or Enum")
        for c in values:                                                                             # (an unordered_set[uint8_t])
            if not 0 <= c <= 255:
                raise OverflowError("class %r does not fit in uint8" % (c,))
        self._classes = sorted(values)
        if isinstance(background, Enum):                                                             # :965-967
            background = background.value
        background = background if background >= 0 else 256 + background
        if not 0 <= background <= 255:
            raise OverflowError("background %r does not fit in uint8" % (background,))
        self._background = int(background)
        self._min_points = int(min_points)
        self._stats = SegmentationStats()
        self._stats.initialize(self._classes)
        if len(self._classes) > 255:                                                                 # :972-973
            raise ValueError("Only support up to 255 different categories!")
        mask = [0] * 8                                                                               # d3d_segeval's 256-bit mask
        for c in self._classes:
            mask[c >> 5] |= 1 << (c & 31)
        self._mask = tuple(mask)

    def reset(self):
        self._stats.initialize(self._classes)

    def calc_stats(self, gt_labels, pred_labels, gt_ids=None, pred_ids=None):
        """-> SegmentationStats of one frame (:1077-1095).  Semantic counts only unless both id arrays are given (uint16).
        numpy arrays (the reference's inputs) or torch tensors; device tensors are read where they are."""
        n = len(gt_labels)
        return self._calc(gt_labels, pred_labels, gt_ids, pred_ids, np.array([0, n], np.int64))[0]

    def calc_stats_batch(self, gt_labels, pred_labels, gt_ids=None, pred_ids=None, frame_offsets=None):
        """Extension (not in the reference): the stats of F frames stacked along the points, frame f = points
        frame_offsets[f] .. frame_offsets[f + 1] - 1 (F + 1 non-decreasing offsets from 0 to the number of points).  -> list of F
        SegmentationStats, each equal to calc_stats of its frame; up to 65535 frames go in one device call."""
        n = len(gt_labels)
        if frame_offsets is None:
            raise ValueError("frame_offsets is required")
        off, = _frame_offsets("frame_offsets must rise from 0 to the number of points", (frame_offsets, n))
        return self._calc(gt_labels, pred_labels, gt_ids, pred_ids, off)

    def _calc(self, gt_labels, pred_labels, gt_ids, pred_ids, off):
        pano = gt_ids is not None and pred_ids is not None                                           # :1087-1093
        if pano and not (_is_u16(gt_ids) and _is_u16(pred_ids)):
            raise ValueError("Please convert ids to uint16!")
        n, frames = len(gt_labels), len(off) - 1
        if len(pred_labels) != n or (pano and (len(gt_ids) != n or len(pred_ids) != n)):
            raise ValueError("labels and ids must have one entry per point")
        if frames == 0:
            return []
        dev = device_of(gt_labels, pred_labels, gt_ids, pred_ids)
        gl = _seg_array(gt_labels, np.uint8, torch.uint8, dev, "gt_labels")
        pl = _seg_array(pred_labels, np.uint8, torch.uint8, dev, "pred_labels")
        gi = _seg_array(gt_ids, np.uint16, torch.uint16, dev, "gt_ids") if pano else None
        pi = _seg_array(pred_ids, np.uint16, torch.uint16, dev, "pred_ids") if pano else None
        lib = _lib.load()
        mask = (ctypes.c_uint32 * 8)(*self._mask)
        out = torch.empty((len(_SEG_FIELDS), frames, 256), dtype=torch.int32, device=dev)
        for f0 in range(0, frames, _SEG_MAX_FRAMES):
            f1 = min(frames, f0 + _SEG_MAX_FRAMES)
            p0, p1 = int(off[f0]), int(off[f1])
            foff = torch.from_numpy(off[f0:f1 + 1] - p0).to(dev)
            ws_bytes = lib.d3d_segeval_workspace_bytes(p1 - p0, f1 - f0)
            ws = _lib.workspace(ws_bytes, dev)

            def at(t):
                return _lib.ptr(t[p0:p1]) if t is not None and p1 > p0 else None
            rows = [_lib.ptr(out[k, f0:f1]) for k in range(len(_SEG_FIELDS))]
            st = lib.d3d_segeval(at(gl), at(pl), at(gi), at(pi),
                                 _lib.ptr(foff), p1 - p0, f1 - f0, mask, self._background, self._min_points,
                                 *rows, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            _lib.check(st, "d3d_segeval")
        res = out.cpu().numpy()
        cum = res[-1].view(np.float32)
        stats = []
        for f in range(frames):
            s = SegmentationStats()
            for i, k in enumerate(_SEG_FIELDS[:-1]):
                setattr(s, k, {c: int(res[i, f, c]) for c in self._classes})
            s.cumiou = {c: float(cum[f, c]) for c in self._classes}
            stats.append(s)
        return stats

    def add_stats(self, stats):
        """:1097-1106 (cumiou summed in fp32 like the reference's float map)"""
        for k in self._classes:
            for name in _SEG_FIELDS[:-1]:
                getattr(self._stats, name)[k] += getattr(stats, name)[k]
            self._stats.cumiou[k] = _f32(np.float32(self._stats.cumiou[k]) + np.float32(stats.cumiou[k]))

    def get_stats(self):
        """Summarize current state of the benchmark counters"""
        return self._stats

    def _typed(self, d):
        if self._class_type is None:
            return dict(d)
        return {self._class_type(k): v for k, v in d.items()}

    def tp(self, instance=False):
        return self._typed(self._stats.itp if instance else self._stats.tp)

    def fp(self, instance=False):
        return self._typed(self._stats.ifp if instance else self._stats.fp)

    def fn(self, instance=False):
        return self._typed(self._stats.ifn if instance else self._stats.fn)

    def _key(self, k):
        return k if self._class_type is None else self._class_type(k)

    def iou(self, instance=False):
        """:1144-1160, fp32 arithmetic; NaN without a denominator"""
        result = {}
        s = self._stats
        for k in self._classes:
            if instance:
                d = np.float32(s.itp[k])
                v = _f32(np.float32(s.cumiou[k]) / d) if s.itp[k] > 0 else math.nan
            else:
                d = np.float32(s.tp[k] + s.fp[k] + s.fn[k])
                v = _f32(np.float32(s.tp[k]) / d) if d > 0 else math.nan
            result[self._key(k)] = v
        return result

    def sq(self):
        """Segmentation Quality (SQ) in panoptic segmentation"""
        return self.iou(instance=True)

    def rq(self):
        """Recognition Quality (RQ) in panoptic segmentation (:1166-1177: the denominator in double, stored as float)"""
        result = {}
        s = self._stats
        for k in self._classes:
            d = np.float32(s.itp[k] + s.ifp[k] * 0.5 + s.ifn[k] * 0.5)
            result[self._key(k)] = _f32(np.float32(s.itp[k]) / d) if d > 0 else math.nan
        return result

    def pq(self):
        """Panoptic Quality (PQ) in panoptic segmentation"""
        sq, rq = self.sq(), self.rq()
        return {k: sq[k] * rq[k] for k in sq}

    def summary(self):
        """:1184-1213"""
        lines = []

        def mean_wo_nan(values):
            valid = [v for v in values if not math.isnan(v)]
            if len(valid) == 0:
                return math.nan
            return sum(valid) / len(valid)

        lines.append("========== Benchmark Summary ==========")
        iou = self.iou()
        sq, rq, pq = self.sq(), self.rq(), self.pq()
        for k in self._classes:
            if k == self._background:
                continue
            typed_k = self._key(k)
            name = str(k).rjust(4, " ") if self._class_type is None else typed_k.name.rjust(20, " ")
            if math.isnan(pq[typed_k]):
                lines.append("%s: iou=%.3f" % (name, iou[typed_k]))
            else:
                lines.append("%s: iou=%.3f, sq=%.3f, rq=%.3f, pq=%.3f" % (name,
                             iou[typed_k], sq[typed_k], rq[typed_k], pq[typed_k]))
        lines.append("mean IoU: %.4f" % mean_wo_nan(iou.values()))
        if not math.isnan(mean_wo_nan(pq.values())):
            lines.append("mean SQ: %.4f" % mean_wo_nan(sq.values()))
            lines.append("mean RQ: %.4f" % mean_wo_nan(rq.values()))
            lines.append("mean PQ: %.4f" % mean_wo_nan(pq.values()))
        lines.append("========== Summary End ==========")
        return "\n".join(lines)


class _TrackFrame(ctypes.Structure):
    """include/d3d_hip.h: D3DTrackFrame"""
    _fields_ = [(k, ctypes.c_void_p) for k in ("dt_boxes", "cache", "dt_cls", "gt_cls", "dt_tid", "gt_tid", "dt_stid", "dt_srow",
                                               "gt_stid", "gt_srow", "dt_perm", "row_off")] + \
               [(k, ctypes.c_int64) for k in ("n", "m", "n_total", "capacity")]


def _tid_counts_merge(a, b):
    """(tids u64[k], counts[..., k]) + (tids, counts) -> the union, counts added (the reference's `+=` on unordered_maps)"""
    u = np.union1d(a[0], b[0]).astype(np.uint64)
    c = np.zeros(a[1].shape[:-1] + (len(u),), np.int64)
    c[..., np.searchsorted(u, a[0])] += a[1]
    c[..., np.searchsorted(u, b[0])] += b[1]
    return u, c


class TrackingEvalStats:
    """Tracking stats summary of an evaluation step (benchmarks.pyx:449-486): the detection counts (ngt, ndt, tp, fp, fn,
    acc_*) plus id_switches / fragments per class and threshold, and the frame counts of the track ids.  The reference keeps
    the latter as hash maps tid -> count; here they are sorted arrays: ngt_ids[c] = (tids u64[k], counts i64[k]),
    ngt_tracked[c] / ndt_ids[c] = (tids u64[k], counts i64[T, k]) -- a tid with count 0 at a threshold is not in that
    threshold's map.  as_object() builds the reference's layout."""

    def initialize(self, classes, nsamples):
        T = nsamples
        self.ngt = {c: 0 for c in classes}
        for k in _COUNT_FIELDS + ("id_switches", "fragments"):
            setattr(self, k, {c: [0] * T for c in classes})
        for k in _ACC_FIELDS:
            setattr(self, k, {c: [math.nan] * T for c in classes})
        empty = np.zeros((0,), np.uint64)
        self.ngt_ids = {c: (empty, np.zeros((0,), np.int64)) for c in classes}
        self.ngt_tracked = {c: (empty, np.zeros((T, 0), np.int64)) for c in classes}
        self.ndt_ids = {c: (empty, np.zeros((T, 0), np.int64)) for c in classes}
        return self

    def as_object(self):
        """:476-486 (whose `ret` is never returned): the tid maps become the lists of their keys, as list() of the
        converted maps gives them -- ascending here"""
        def keys(entry):
            tids, counts = entry
            if counts.ndim == 1:
                return [int(x) for x in tids[counts > 0]]
            return [[int(x) for x in tids[row > 0]] for row in counts]
        plain = ("ngt",) + _COUNT_FIELDS[1:] + _COUNT_FIELDS[:1] + _ACC_FIELDS + ("id_switches", "fragments")   # (ndt after fn, :478)
        obj = {k: dict(getattr(self, k)) for k in plain}
        for k in ("ngt_ids", "ngt_tracked", "ndt_ids"):
            obj[k] = {c: keys(v) for c, v in getattr(self, k).items()}
        return obj

    def __repr__(self):
        return "TrackingEvalStats(%r)" % (self.as_object(),)


def _host_rows(x, dtype, cols):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    return np.ascontiguousarray(x, dtype=dtype).reshape((-1, cols) if cols else (-1,))


def _host_tids(x, what):
    if torch.is_tensor(x):
        if x.dtype not in (torch.int64, torch.uint64):
            raise ValueError("%s: expected 64-bit integer track ids, got %s" % (what, x.dtype))
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype not in (np.uint64, np.int64):
        raise ValueError("%s: expected uint64 / int64 track ids, got %s" % (what, x.dtype))
    return np.ascontiguousarray(x.reshape(-1)).view(np.uint64)


def _aligned(nbytes):
    return (nbytes + 255) // 256 * 256


class TrackingEvaluator(DetectionEvaluator):
    """Benchmark for object tracking (benchmarks.pyx:488-890).  Targets association is done by score sorting, with the
    assignments of the previous frame carried over per score threshold.

    Boxes are [n,9] rows as for DetectionEvaluator; their track ids come as separate arrays (uint64 / int64, numpy or
    tensors).  The carried state lives on the device: a frame is d3d_match_distance + d3d_track_frame (prepare, the literal
    association of every threshold, update) without a host round trip, so calc_stats_sequence queues whole sequences and
    fetches once.  Extension beyond the reference: calc_stats_sequence."""

    def __init__(self, classes, min_overlaps, pr_sample_count=40, min_score=0, pr_sample_scale="log10"):
        super().__init__(classes, min_overlaps, pr_sample_count=pr_sample_count, min_score=min_score,
                         pr_sample_scale=pr_sample_scale)
        self._dev = None
        self._state = None              # two device buffers of d3d_track_state_bytes(self._cap, T), self._state[self._cur] current
        self._cap, self._cur = 0, 0
        self._host_state = None          # (capacity, bytes) of a state that was pickled, uploaded at the next frame

    def _new_stats(self):
        return TrackingEvalStats().initialize(self._classes, self._pr_nsamples)

    def reset(self):
        DetectionEvaluator.reset(self)
        self._host_state = None
        if self._state is not None:
            self._state[self._cur][:4 * self._pr_nsamples].zero_()        # count[T] = 0: no carried pairs

    # ------------------------------------------------------------------ device state
    def _state_views(self, buf, cap):
        T = self._pr_nsamples
        o1 = _aligned(4 * T)
        o2 = o1 + _aligned(8 * T * cap)
        o3 = o2 + _aligned(8 * T * cap)
        o4 = o3 + _aligned(4 * T * cap)
        return (buf[:4 * T].view(torch.int32), buf[o1:o1 + 8 * T * cap].view(torch.int64).view(T, cap),
                buf[o2:o2 + 8 * T * cap].view(torch.int64).view(T, cap), buf[o3:o3 + 4 * T * cap].view(torch.int32).view(T, cap),
                buf[o4:o4 + 4 * T * cap].view(torch.int32).view(T, cap))

    def _ensure_state(self, dev, m):
        """two state buffers of capacity >= m on `dev` (grown with the pairs copied over: no synchronisation)"""
        lib = _lib.load()
        T = self._pr_nsamples
        if self._state is not None and self._dev != dev:
            raise ValueError("TrackingEvaluator: frames of one sequence must stay on one device")
        self._dev = dev
        if self._host_state is not None:
            cap, raw = self._host_state
            self._host_state = None
            buf = torch.from_numpy(raw.copy()).to(dev)
            self._state = [buf, torch.zeros_like(buf)]
            self._cap, self._cur = cap, 0
        if self._state is not None and m <= self._cap:
            return
        cap = max(m, 2 * self._cap, 64)
        nbytes = lib.d3d_track_state_bytes(cap, T)
        new = [torch.zeros((nbytes,), dtype=torch.uint8, device=dev) for _ in range(2)]
        if self._state is not None:
            old, dst = self._state_views(self._state[self._cur], self._cap), self._state_views(new[0], cap)
            dst[0].copy_(old[0])
            for a, b in zip(dst[1:], old[1:]):
                a[:, :self._cap].copy_(b)
        self._state, self._cap, self._cur = new, cap, 0

    def __getstate__(self):
        d = dict(self.__dict__)
        if self._state is not None:                      # the carried assignments travel with the evaluator
            d["_host_state"] = (self._cap, self._state[self._cur].cpu().numpy())
        d["_state"], d["_dev"], d["_cap"], d["_cur"] = None, None, 0, 0
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    # ------------------------------------------------------------------ calc_stats
    def calc_stats(self, gt_boxes, dt_boxes, gt_tids, dt_tids):
        """-> TrackingEvalStats of one frame (:536-723); updates the carried assignments, adds nothing to the totals
        (add_stats does).  Both box sets must be in the same frame."""
        gt = _host_rows(gt_boxes, np.float32, 9)
        dt = _host_rows(dt_boxes, np.float32, 9)
        h = self._prepare_host(gt, dt, _host_tids(gt_tids, "gt_tids"), _host_tids(dt_tids, "dt_tids"))
        return self._run([h], device_of(gt_boxes, dt_boxes, gt_tids, dt_tids))[0]

    def calc_stats_sequence(self, gt_boxes, dt_boxes, gt_tids, dt_tids, gt_frame_offsets, dt_frame_offsets):
        """Extension (not in the reference): F frames stacked, frame f = gt rows gt_frame_offsets[f] .. gt_frame_offsets[f + 1]
        and dt rows dt_frame_offsets[f] .. dt_frame_offsets[f + 1] (F + 1 offsets each, rising from 0 to the number of rows).
        -> list of F TrackingEvalStats, equal to F successive calc_stats calls; the frames are queued without a host
        synchronisation between them and the results fetched once."""
        gt = _host_rows(gt_boxes, np.float32, 9)
        dt = _host_rows(dt_boxes, np.float32, 9)
        gtid, dtid = _host_tids(gt_tids, "gt_tids"), _host_tids(dt_tids, "dt_tids")
        if len(gtid) != len(gt) or len(dtid) != len(dt):
            raise ValueError("one track id per box is required")
        go, do = _frame_offsets("frame offsets must rise from 0 to the number of boxes",
                                (gt_frame_offsets, len(gt)), (dt_frame_offsets, len(dt)))
        hs = [self._prepare_host(gt[go[f]:go[f + 1]], dt[do[f]:do[f + 1]], gtid[go[f]:go[f + 1]], dtid[do[f]:do[f + 1]])
              for f in range(len(go) - 1)]
        return self._run(hs, device_of(gt_boxes, dt_boxes, gt_tids, dt_tids)) if hs else []

    def calc_stats_batch(self, *args, **kwargs):
        """not for tracking: the frames of a sequence depend on each other and need track ids"""
        raise TypeError("TrackingEvaluator has no calc_stats_batch (frames carry track ids and depend on their predecessors): "
                        "use calc_stats_sequence")

    def _prepare_host(self, gt, dt, gtid, dtid):
        """what the host knows of a frame before the device runs: the class slots, the selections, the orders, the tid tables"""
        if len(gtid) != len(gt) or len(dtid) != len(dt):
            raise ValueError("one track id per box is required")
        if len(np.unique(gtid)) != len(gtid) or len(np.unique(dtid)) != len(dtid):
            raise ValueError("track ids must be unique among the boxes of a frame")
        gslot, dslot = _class_slots(self._classes, gt), _class_slots(self._classes, dt)
        score = dt[:, 1]
        sel = (dslot >= 0)[None, :] & ~(score[None, :] < self._pr_thresholds[:, None])          # [T, n]  (:588-593)
        if np.any(sel.any(0) & (dtid == 0)):
            raise AssertionError("Tracking id should be greater than 0 for a valid object!")      # :597
        row_off = np.zeros((self._pr_nsamples + 1,), np.int64)
        np.cumsum(sel.sum(1), out=row_off[1:])
        perm = np.flip(np.argsort(score, kind="stable")).astype(np.int32)                        # matcher.pyx:146
        go, do = np.argsort(gtid, kind="stable"), np.argsort(dtid, kind="stable")
        return dict(gt=gt, dt=dt, gtid=gtid, dtid=dtid, gslot=gslot, dslot=dslot, sel=sel, row_off=row_off, perm=perm,
                    gt_stid=gtid[go], gt_srow=go.astype(np.int32), dt_stid=dtid[do], dt_srow=do.astype(np.int32))

    def _run(self, hs, dev):
        """the device chain of every frame of `hs` (_prepare_host), queued in order; one fetch at the end"""
        lib = _lib.load()
        T, C = self._pr_nsamples, len(self._classes)
        # everything the device reads, in one upload: the thresholds, the classes' distances, then per frame [dt boxes f32 |
        # row_off i64 | 4 tid arrays u64 | 5 index arrays i32]
        inputs = (("dt", "dt_boxes"), ("row_off", "row_off"), ("dtid", "dt_tid"), ("gtid", "gt_tid"), ("dt_stid", "dt_stid"),
                  ("gt_stid", "gt_stid"), ("dslot", "dt_cls"), ("gslot", "gt_cls"), ("dt_srow", "dt_srow"), ("gt_srow", "gt_srow"),
                  ("perm", "dt_perm"))                          # (_prepare_host's key, _TrackFrame's field)
        pieces = [self._pr_thresholds, np.array([np.float32(self._max_distance[c]) for c in self._classes], np.float32)]
        pieces += [h[k] for h in hs for k, _ in inputs]
        sizes = [(len(h["dt"]), len(h["gt"])) for h in hs]
        cache_at, out_at, cpos, opos = [], [], 0, 0
        for n, m in sizes:                                      # the caches; the outputs assign, iou [T, m] and counts [T, 3, C]
            cache_at.append(cpos)
            cpos += n * m
            out_at.append(opos)
            opos += 2 * T * m + 3 * T * C
        with torch.cuda.device(dev):
            blob, addr = _upload(dev, pieces)
            gts = [torch.from_numpy(h["gt"]) for h in hs]
            gt_dev = torch.cat(gts).to(dev) if sum(len(g) for g in gts) else None
            caches = torch.empty((max(cpos, 1),), dtype=torch.float32, device=dev)
            out = torch.empty((max(opos, 1),), dtype=torch.int32, device=dev)
            self._ensure_state(dev, max(m for _, m in sizes))
            ws_bytes = max(max(lib.d3d_track_workspace_bytes(n, m, T, int(h["row_off"][-1])),
                               lib.d3d_iou3d_workspace_bytes(n, m)) for (n, m), h in zip(sizes, hs))
            ws = _lib.workspace(ws_bytes, dev)
            stream = _lib.stream_ptr()
            g0 = 0
            fr = _TrackFrame()
            for i, ((n, m), h, ca, oa) in enumerate(zip(sizes, hs, cache_at, out_at)):
                lay = addr[2 + len(inputs) * i:2 + len(inputs) * (i + 1)]
                for (_, field), at in zip(inputs, lay):
                    setattr(fr, field, at)
                cache_ptr = caches.data_ptr() + 4 * ca
                if n and m:
                    rc = lib.d3d_match_distance(ctypes.c_void_p(lay[0]), n, ctypes.c_void_p(gt_dev.data_ptr() + 36 * g0), m,
                                                1, ctypes.c_void_p(cache_ptr), _lib.ptr(ws), ws.numel(), stream)
                    _lib.check(rc, "match_distance")
                g0 += m
                fr.cache = cache_ptr if n and m else None
                fr.n, fr.m, fr.n_total, fr.capacity = n, m, int(h["row_off"][-1]), self._cap
                optr = out.data_ptr() + 4 * oa
                rc = lib.d3d_track_frame(ctypes.addressof(fr), ctypes.c_void_p(addr[0]), T, ctypes.c_void_p(addr[1]),
                                         C, _lib.ptr(self._state[self._cur]), _lib.ptr(self._state[1 - self._cur]),
                                         ctypes.c_void_p(optr), ctypes.c_void_p(optr + 4 * T * m),
                                         ctypes.c_void_p(optr + 8 * T * m), _lib.ptr(ws), ws.numel(), stream)
                _lib.check(rc, "track_frame")
                self._cur ^= 1
            res = out.cpu().numpy()
        return [self._frame_stats(h, res[oa:oa + 2 * T * len(h["gt"]) + 3 * T * C]) for h, oa in zip(hs, out_at)]

    def _frame_stats(self, h, res):
        """the TrackingEvalStats of a frame from the device's per-threshold assignment and counters (:617-723)"""
        T, C, classes = self._pr_nsamples, len(self._classes), self._classes
        gt, dt, gslot, dslot, sel = h["gt"], h["dt"], h["gslot"], h["dslot"], h["sel"]
        m = len(gt)
        assign = res[:T * m].reshape(T, m)
        iou = res[T * m:2 * T * m].view(np.float32).reshape(T, m)
        counts = res[2 * T * m:].reshape(T, 3, C)
        st = TrackingEvalStats().initialize(classes, T)
        tracked = (assign >= 0) & (gslot >= 0)[None, :]
        tt, jj = np.nonzero(tracked)
        tp, acc = _bin_means(gslot[jj].astype(np.int64) * T + tt, (C, T), _pair_terms(gt[jj], dt[assign[tt, jj]], iou[tt, jj]))
        for i, c in enumerate(classes):
            gi = np.nonzero(gslot == i)[0]
            gi = gi[np.argsort(h["gtid"][gi], kind="stable")]
            di = np.nonzero(dslot == i)[0]
            di = di[np.argsort(h["dtid"][di], kind="stable")]
            st.ngt[c] = len(gi)
            st.ngt_ids[c] = (h["gtid"][gi], np.ones((len(gi),), np.int64))
            st.ngt_tracked[c] = (h["gtid"][gi], tracked[:, gi].astype(np.int64))
            st.ndt_ids[c] = (h["dtid"][di], sel[:, di].astype(np.int64))
            st.ndt[c] = sel[:, di].sum(1).tolist()
            st.tp[c] = tp[i].tolist()
            st.fn[c] = (len(gi) - tp[i]).tolist()
            st.fp[c] = counts[:, 0, i].tolist()
            st.id_switches[c] = counts[:, 1, i].tolist()
            st.fragments[c] = counts[:, 2, i].tolist()
            for name, a in zip(_ACC_FIELDS, acc):
                getattr(st, name)[c] = a[i].tolist()
        return st

    # ------------------------------------------------------------------ accumulation and metrics
    def add_stats(self, stats):
        """:725-756"""
        DetectionEvaluator.add_stats(self, stats)
        s = self._stats
        for k in self._classes:
            s.ngt_ids[k] = _tid_counts_merge(s.ngt_ids[k], stats.ngt_ids[k])
            s.ngt_tracked[k] = _tid_counts_merge(s.ngt_tracked[k], stats.ngt_tracked[k])
            s.ndt_ids[k] = _tid_counts_merge(s.ndt_ids[k], stats.ndt_ids[k])
            s.id_switches[k] = [a + int(b) for a, b in zip(s.id_switches[k], stats.id_switches[k])]
            s.fragments[k] = [a + int(b) for a, b in zip(s.fragments[k], stats.fragments[k])]

    def id_switches(self, score=math.nan):
        """Return ID switch count. If score is not specified, return the median value"""
        return self._at(self._stats.id_switches, score)

    def fragments(self, score=math.nan):
        """Return fragments count. If score is not specified, return the median value"""
        return self._at(self._stats.fragments, score)

    def gt_traj_count(self):
        """Return total ground-truth trajectory count. gt() will return total bounding box count"""
        return {self._key(k): int(np.count_nonzero(self._stats.ngt_ids[k][1])) for k in self._classes}

    def _calc_frame_ratio(self, score, frame_ratio_threshold, high_pass, return_all):
        """:790-819: per class, the share of gt trajectories tracked in more (high_pass) / fewer than the threshold's share of
        their frames (fp32 ratio); divided by the number of gt trajectories (ZeroDivisionError without one, as there)"""
        thr = np.float32(frame_ratio_threshold)
        idx = list(range(self._pr_nsamples)) if return_all else [self._get_score_idx(score)]
        r = {}
        for k in self._classes:
            gids, gcnt = self._stats.ngt_ids[k]
            tids, tcnt = self._stats.ngt_tracked[k]
            total = gcnt[np.searchsorted(gids, tids)] if len(tids) else np.zeros((0,), np.int64)
            vals = []
            for i in idx:
                on = tcnt[i] > 0
                ratio = (tcnt[i][on].astype(np.float64) / total[on]).astype(np.float32)
                hit = ratio > thr if high_pass else ratio < thr
                vals.append(float(int(hit.sum())) / len(gids))
            r[self._key(k)] = vals if return_all else vals[0]
        return r

    def tracked_ratio(self, score=math.nan, frame_ratio_threshold=0.8, return_all=False):
        """Return the ratio of mostly tracked trajectories (tracked in more than frame_ratio_threshold of their frames)"""
        return self._calc_frame_ratio(score, frame_ratio_threshold, True, return_all)

    def lost_ratio(self, score=math.nan, frame_ratio_threshold=0.2, return_all=False):
        """Return the ratio of mostly lost trajectories (tracked in fewer than frame_ratio_threshold of their frames)"""
        return self._calc_frame_ratio(score, frame_ratio_threshold, False, return_all)

    def mota(self, score=math.nan):
        """Return the MOTA metric defined by the CLEAR MOT metrics (:835-841). For MOTP equivalents, see acc_* properties"""
        i, s = self._get_score_idx(score), self._stats
        r = {}
        for k in self._classes:
            with np.errstate(invalid="ignore", divide="ignore"):
                r[self._key(k)] = float(1 - np.float64(s.fp[k][i] + s.fn[k][i] + s.id_switches[k][i]) / np.float64(s.ngt[k]))
        return r

    def summary(self, score_thres=0.8, tracked_ratio_thres=0.8, lost_ratio_thres=0.2, note=None, verbose=False):
        """Print default summary (into returned string) (:843-890); int classes print as the int"""
        score_thres = _f32(score_thres)
        tracked_ratio_thres, lost_ratio_thres = _f32(tracked_ratio_thres), _f32(lost_ratio_thres)
        score_idx = self._get_score_idx(score_thres)
        s = self._stats
        lines = [""]
        precision, recall = self.precision(score_thres), self.recall(score_thres)
        fscore, ap = self.fscore(return_all=True), self.ap()
        mlt = self.tracked_ratio(score_thres, tracked_ratio_thres)
        mll = self.lost_ratio(score_thres, lost_ratio_thres)
        mota = self.mota(score_thres)
        if note:
            lines.append("========== Benchmark Summary (%s) ==========" % note)
        else:
            lines.append("========== Benchmark Summary ==========")
        for k in self._classes:
            typed_k = self._key(k)
            if verbose:
                lines.append("Results for %s:" % self._name(k))
                lines.append("\tTotal processed targets:\t%d gt boxes, %d dt boxes" % (s.ngt[k], max(s.ndt[k])))
                lines.append("\tTotal processed trajectories:\t%d gt tracklets, %d dt tracklets" % (
                    self.gt_traj_count()[typed_k], max(int(np.count_nonzero(row)) for row in s.ndt_ids[k][1])))
                lines.append("\tPrecision (score > %.2f):\t%.3f" % (score_thres, precision[typed_k]))
                lines.append("\tRecall (score > %.2f):\t\t%.3f" % (score_thres, recall[typed_k]))
                lines.append("\tMax F1:\t\t\t\t%.3f" % max(fscore[typed_k]))
                lines.append("\tAP:\t\t\t\t%.3f" % ap[typed_k])
                lines.append("")
                lines.append("\tID switches (score > %.2f):\t\t\t%d" % (score_thres, s.id_switches[k][score_idx]))
                lines.append("\tFragments (score > %.2f):\t\t\t%d" % (score_thres, s.fragments[k][score_idx]))
                lines.append("\tMOTA (score > %.2f):\t\t\t\t%.2f" % (score_thres, mota[typed_k]))
                lines.append("\tMostly tracked (score > %.2f, ratio > %.2f):\t%.3f" % (
                    score_thres, tracked_ratio_thres, mlt[typed_k]))
                lines.append("\tMostly lost (score > %.2f, ratio < %.2f):\t%.3f" % (
                    score_thres, lost_ratio_thres, mll[typed_k]))
                lines.append("")
                self._summary_accuracy(lines, k, score_thres, score_idx)
            else:
                lines.append("Results for %s: AP=%.3f, MOTA=%.3f" % (self._name(k), ap[typed_k], mota[typed_k]))
        lines.append("mAP: %.3f" % np.mean(list(ap.values())))
        lines.append("========== Summary End ==========")
        return "\n".join(lines)


__all__ = ["DetectionEvaluator", "SegmentationEvaluator", "SegmentationStats", "TrackingEvalStats", "TrackingEvaluator"]
