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
"""
import ctypes
import math
from enum import Enum

import numpy as np
import torch

from . import _lib
from .tracking.matcher import DistanceTypes, ReferenceAssociation, prepare_boxes, score_match
from .utils import Dict


class DetectionEvaluator:
    """Benchmark for object detection; targets association is done by score sorting (benchmarks.pyx:84-149)."""

    def __init__(self, classes, min_overlaps, pr_sample_count=40, min_score=0, pr_sample_scale="log10", reference_compat=True):
        self.reference_compat = bool(reference_compat)
        classes = list(classes) if isinstance(classes, (list, tuple)) else [classes]
        assert len(classes) > 0
        self._classes = [int(getattr(c, "value", c)) for c in classes]
        if isinstance(min_overlaps, (list, tuple)):
            self._max_distance = {c: 1 - v for c, v in zip(self._classes, min_overlaps)}            # :114-115
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

    @property
    def score_thresholds(self):
        return self._pr_thresholds

    def calc_stats(self, gt_boxes, dt_boxes):
        """-> Dict(ngt{c}, ndt{c}[T], tp, fp, fn, acc_iou{c}[T], acc_angular, acc_dist, acc_box, acc_var) as
        DetectionEvalStats (benchmarks.pyx:60-82, 178-283); both box sets must be in the same frame"""
        gt = np.ascontiguousarray(gt_boxes, dtype=np.float32).reshape(-1, 9)
        dt = np.ascontiguousarray(dt_boxes, dtype=np.float32).reshape(-1, 9)
        T, classes = self._pr_nsamples, self._classes
        thr = self._pr_thresholds
        gt_tag, dt_tag = gt[:, 0].astype(np.int64), dt[:, 0].astype(np.int64)
        dt_score = dt[:, 1]
        out = Dict(ngt={}, ndt={}, tp={}, fp={}, fn={}, acc_iou={}, acc_angular={}, acc_dist={}, acc_box={}, acc_var={})
        if self.reference_compat:
            return self._calc_stats_per_threshold(gt, dt, out)
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
            matched = dm >= 0
            iou = np.zeros((len(gt),), np.float32)
        partner = np.where(matched, dm, 0)
        # a ground-truth box is a true positive at threshold t iff its detection is selected there (score >= t)  (:220-238)
        gscore = np.where(matched, dt_score[partner] if len(dt) else 0.0, -np.inf)
        dist = np.linalg.norm(gt[:, 2:5] - dt[partner, 2:5], axis=1) if len(dt) else np.zeros(len(gt))          # :244
        box = np.linalg.norm(gt[:, 5:8] - dt[partner, 5:8], axis=1) if len(dt) else np.zeros(len(gt))           # :245
        dyaw = (gt[:, 8] - dt[partner, 8]) if len(dt) else np.zeros(len(gt))
        ang = np.abs((dyaw + np.pi) % (2 * np.pi) - np.pi) / np.pi                                     # quatdiff of two yaw rotations / pi (:247-248)
        dmatched = sm >= 0
        vals = np.stack([iou, ang, dist, box]).astype(np.float64)                                      # [4, m]

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
            out.acc_iou[c], out.acc_angular[c] = means[0].tolist(), means[1].tolist()
            out.acc_dist[c], out.acc_box[c] = means[2].tolist(), means[3].tolist()
            # no variances travel in the [n,9] arrays: orientation_var = 0 -> -inf per match (:250-258), NaN without one
            out.acc_var[c] = np.where(tp > 0, -np.inf, np.nan).astype(np.float32).tolist()
        return out


    def _calc_stats_per_threshold(self, gt, dt, out):
        """benchmarks.pyx:188-283 as written: select the detections of a threshold, associate (the literal pairing), count"""
        T, classes, thr = self._pr_nsamples, self._classes, self._pr_thresholds
        gt_tag, dt_tag = gt[:, 0].astype(np.int64), dt[:, 0].astype(np.int64)
        dt_score = dt[:, 1]
        gt_idx = np.nonzero(np.isin(gt_tag, classes))[0]                                              # :205-212
        dt_in = np.isin(dt_tag, classes)
        for c in classes:
            out.ngt[c] = int((gt_tag == c).sum())
            for k in ("ndt", "tp", "fp", "fn"):
                out[k][c] = [0] * T
            for k in ("acc_iou", "acc_angular", "acc_dist", "acc_box", "acc_var"):
                out[k][c] = [float("nan")] * T
        cache = prepare_boxes(dt, gt, DistanceTypes.RIoU) if len(gt) and len(dt) else None             # :188-189
        # the 40 associations share what does not depend on the threshold (the ground truths' columns of the cache, which pairs are
        # acceptable) and go to the device as batched calls (ReferenceAssociation.match_many: one for a frame, a few for config 4's
        # 20 k x 5 k), nothing read back in between; the results are fetched together
        assoc = gt_idx_t = None
        if cache is not None and len(gt_idx):
            assoc = ReferenceAssociation(cache, dt_score, dt_tag, gt_tag, self._max_distance, gt_idx)
            gt_idx_t = torch.from_numpy(gt_idx).to(cache.device)
        sel = dt_in[None, :] & ~(dt_score[None, :] < thr[:, None])                                   # [T, n]: :219-228 (`score < thres`: skip)
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
        # the counts and means of :236-283 for all thresholds at once: the K matched (threshold, ground truth) pairs as flat arrays,
        # per-threshold counts and float64 sums by bincount (the arithmetic of one pair is unchanged: float32 terms, their sum in
        # float64, one division, rounded to float32)
        tt, jj = np.nonzero(dm_g >= 0)
        terms, gcls = {}, np.zeros((0,), np.int64)
        if len(tt):
            gi, d_of = gt_idx[jj], dm_g[tt, jj]
            ga, da = gt[gi], dt[d_of]                                                                  # [K, 9]
            dp, db = ga[:, 2:5] - da[:, 2:5], ga[:, 5:8] - da[:, 5:8]
            dyaw = ga[:, 8] - da[:, 8]
            terms = dict(acc_iou=iou_all[tt, jj],
                         acc_angular=np.abs((dyaw + np.pi) % (2 * np.pi) - np.pi) / np.pi,              # :247-248
                         # (np.linalg.norm(., axis=1) spelled out -- sqrt(add.reduce(x * x)) over three terms, the same bits)
                         acc_dist=np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2]),   # :244
                         acc_box=np.sqrt((db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1]) + db[:, 2] * db[:, 2]))    # :245
            gcls = gt_tag[gi]
        unmatched = sm_all < 0
        for c in classes:
            dc = sel & (dt_tag == c)[None, :]
            of_c = gcls == c
            tc = tt[of_c]
            tp = np.bincount(tc, minlength=T)
            out.ndt[c] = dc.sum(1).tolist()
            out.tp[c] = tp.tolist()
            out.fn[c] = (out.ngt[c] - tp).tolist()                                                     # :236-240
            out.fp[c] = (dc & unmatched).sum(1).tolist()                                               # :262-265
            for name, v in terms.items():                                                              # :150-174 (sum / count, fp32)
                ssum = np.bincount(tc, weights=v[of_c].astype(np.float64), minlength=T)
                with np.errstate(invalid="ignore", divide="ignore"):
                    out[name][c] = np.where(tp > 0, (ssum / tp).astype(np.float32), np.float32(np.nan)).tolist()
            # no variances travel in the [n,9] arrays: orientation_var = 0 -> -inf per match (:250-258), NaN without one
            out.acc_var[c] = np.where(tp > 0, -np.inf, np.nan).tolist()
        return out


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


def _seg_device(*tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.device.type == "cuda":
            return t.device
    return _lib.require_gpu()


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
        off = frame_offsets.cpu().numpy() if torch.is_tensor(frame_offsets) else np.asarray(frame_offsets)
        off = off.astype(np.int64).reshape(-1)
        if len(off) < 1 or off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 0):
            raise ValueError("frame_offsets must rise from 0 to the number of points")
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
        dev = _seg_device(gt_labels, pred_labels, gt_ids, pred_ids)
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


__all__ = ["DetectionEvaluator", "SegmentationEvaluator", "SegmentationStats"]
