"""A literal restatement of SegmentationEvaluator.collect_labels / collect_labels_pano (reference d3d/benchmarks.pyx:977-1075)
in Python / numpy: the checker of the GPU path beyond the goldens (large frames, random frames, the frames the golden generator
must not produce).  -> dict field -> {class: value} as SegmentationStats.as_object() (benchmarks.pyx:926-929)."""
import numpy as np


def _zero(classes):
    return dict(tp={c: 0 for c in classes}, fp={c: 0 for c in classes}, fn={c: 0 for c in classes},
                itp={c: 0 for c in classes}, ifp={c: 0 for c in classes}, ifn={c: 0 for c in classes},
                cumiou={c: np.float32(0) for c in classes})


def collect_labels(stats, classes, background, gt_labels, pred_labels):
    """:977-987, as counts over the points (numpy instead of the loop, the same conditions)"""
    g = np.asarray(gt_labels, np.int64)
    p = np.asarray(pred_labels, np.int64)
    for c in classes:
        if c == background:                       # `gt_labels[i] != self._background` / `pred_labels[i] != ...`
            continue
        stats["tp"][c] += int(np.count_nonzero((g == c) & (p == c)))         # :979-981
        stats["fn"][c] += int(np.count_nonzero((g == c) & (p != c)))         # :982-983
        stats["fp"][c] += int(np.count_nonzero((p == c) & (g != c)))         # :984-985


def collect_labels_pano(stats, classes, background, min_points, gt_labels, pred_labels, gt_ids, pred_ids):
    collect_labels(stats, classes, background, gt_labels, pred_labels)      # :993
    g = np.asarray(gt_labels, np.int64)
    p = np.asarray(pred_labels, np.int64)
    cls = np.zeros((256,), bool)
    cls[list(classes)] = True
    bg_key = background << 16                                               # :1000
    gt_key = np.where(cls[g], g << 16 | np.asarray(gt_ids, np.int64), bg_key)          # :1001-1004
    pred_key = np.where(cls[p], p << 16 | np.asarray(pred_ids, np.int64), bg_key)      # :1005-1008
    # counter[gt_key][pred_key], gt_counter, pred_counter (:1010-1027): occurrence counts of the keys
    pairs, inter = np.unique(gt_key << 32 | pred_key, return_counts=True)
    gks, gcs = np.unique(gt_key, return_counts=True)
    pks, pcs = np.unique(pred_key, return_counts=True)
    gt_counter = dict(zip(gks.tolist(), gcs.tolist()))
    pred_counter = dict(zip(pks.tolist(), pcs.tolist()))
    counter = {}
    for k, c in zip(pairs.tolist(), inter.tolist()):
        counter.setdefault(k >> 32, {})[k & 0xffffffff] = c
    pred_unmatched = set(pks.tolist())                                      # :1029-1030

    for gk, row in counter.items():                                         # :1037-1062
        matched = False
        gt_label = gk >> 16
        if gt_label == background:
            continue
        if gt_counter[gk] < min_points:
            continue
        for pk, n_inter in row.items():
            pred_label = pk >> 16
            if pred_label == background:
                continue
            if gt_label != pred_label:
                continue
            # :1053-1056 -- the subtraction only runs after find() failed, i.e. it subtracts the 0 operator[] inserts
            total = np.float32(gt_counter[gk] + pred_counter[pk] - n_inter)
            iou = np.float32(np.float32(n_inter) / total)
            if iou > 0.5:
                stats["itp"][gt_label] += 1
                stats["cumiou"][gt_label] = np.float32(stats["cumiou"][gt_label] + iou)
                matched = True
                pred_unmatched.discard(pk)
        if not matched:
            stats["ifn"][gt_label] += 1

    for pk in pred_unmatched:                                               # :1064-1070
        if pred_counter[pk] < min_points:
            continue
        pred_label = pk >> 16
        if pred_label != background:
            stats["ifp"][pred_label] += 1


def calc_stats(classes, background, min_points, gt_labels, pred_labels, gt_ids=None, pred_ids=None):
    """:1077-1095 for one frame"""
    classes = sorted(set(int(c) for c in classes))
    stats = _zero(classes)
    if gt_ids is None or pred_ids is None:
        collect_labels(stats, classes, background, gt_labels, pred_labels)
    else:
        collect_labels_pano(stats, classes, background, min_points, gt_labels, pred_labels, gt_ids, pred_ids)
    stats["cumiou"] = {c: float(v) for c, v in stats["cumiou"].items()}
    return stats
