"""d3d_amd.tracking.matcher -- BaseMatcher.prepare_boxes + ScoreMatcher of the reference (d3d/tracking/matcher.pyx:12-162)
on arrays: boxes are [n,9] float32 rows (label, score, x, y, z, lx, ly, lz, yaw), the layout Target3DArray.to_numpy produces
(d3d/abstraction.pyx:263-272) and prepare_boxes consumes (matcher.pyx:46-51).  The container classes of d3d.abstraction are
outside this library's scope; everything that is arithmetic runs in HIP kernels (d3d_match_distance, d3d_score_match).
"""
import ctypes
import enum

import numpy as np
import torch

from .. import _lib
from .._rows import device_of


class DistanceTypes(enum.IntEnum):      # matcher.pxd:5-8
    IoU = 1
    RIoU = 2
    Position = 3


def _host(a):
    """tags, scores, flags: numpy arrays, lists, or tensors on any device -> numpy on the host"""
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _threshold_of(distance_threshold, tags):
    """unordered_map<int, float>::operator[] (matcher.pyx:112, :115, :227): the threshold of every tag as fp32, a tag missing from
    the map reads as 0.0"""
    thr = np.zeros((tags.size,), np.float32)
    for tag in set(tags.tolist()):      # (a frame has a handful of classes: cheaper than np.unique's sort)
        thr[tags == tag] = np.float32(float(distance_threshold.get(tag, 0.0)))
    return thr


def _unmatched(dev, n, m, batch=()):
    """(src_match[*batch, n], dst_match[*batch, m]) int32 on the device, every box unmatched (-1)"""
    return tuple(torch.full(tuple(batch) + (k,), -1, dtype=torch.int32, device=dev) for k in (n, m))


def _boxes(a, what):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if isinstance(a, np.ndarray) else a.to(torch.float32)
    if t.dim() != 2 or t.shape[1] != 9:
        raise ValueError("%s should be [n,9] rows of (label, score, x, y, z, lx, ly, lz, yaw)" % what)
    return t


def prepare_boxes(src_arr, dst_arr, distance_metric):
    """the distance cache of BaseMatcher.prepare_boxes (matcher.pyx:25-80): f32[n,m] on the device.
    IoU -> 1 - box3d_iou, RIoU -> 1 - box3dr_iou (dimensions clipped to +-1e3 first, :49-51), Position -> euclidean distance
    of the centres (the reference's cdist over columns 0:3 of these arrays, :82, compares (label, score, x): a slip)."""
    lib = _lib.load()
    metric = DistanceTypes(int(distance_metric))
    src, dst = _boxes(src_arr, "src_boxes"), _boxes(dst_arr, "dst_boxes")
    dev = device_of(src, dst)
    src, dst = src.to(dev).contiguous(), dst.to(dev).contiguous()
    n, m = src.shape[0], dst.shape[0]
    with torch.cuda.device(dev):
        if metric == DistanceTypes.Position:
            return torch.cdist(src[:, 2:5], dst[:, 2:5], compute_mode="donot_use_mm_for_euclid_dist")
        cache = torch.empty((n, m), dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.d3d_iou3d_workspace_bytes(n, m), dev)
        rc = lib.d3d_match_distance(_lib.ptr(src), n, _lib.ptr(dst), m, 1 if metric == DistanceTypes.RIoU else 0, _lib.ptr(cache),
                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    _lib.check(rc, "match_distance")
    return cache


def score_match(distance, src_scores, src_tags, dst_tags, distance_threshold):
    """ScoreMatcher.match over ALL boxes (matcher.pyx:142-162 + match_by_order :90-121): src rows from the best score down,
    each takes the nearest unassigned dst of its own tag with distance <= distance_threshold[tag].  Tags absent from
    `distance_threshold` (or negative) take no part.  Returns (src_match[n], dst_match[m]) int32 tensors on the device,
    -1 = unmatched.  The matching of a score threshold t is this result restricted to the src with score >= t: a box's choice
    only depends on the boxes before it (benchmarks.pyx:218-238 recomputes it per threshold).  Any threshold is exact (rows with
    more than 64 candidates list their 64 nearest and fall back to a sweep of the row).  Ties: equal scores are taken
    in index order, equal distances go to the lower dst index (the reference's argsorts leave both unspecified)."""
    lib = _lib.load()
    dev = distance.device
    n, m = distance.shape
    # host-side preparation in numpy (a frame has a few hundred boxes: tensor ops would each cost more than the arithmetic),
    # shipped to the device in ONE copy: src scores f32, src tags i32, dst tags i32, dst thresholds f32
    st = _host(src_tags).astype(np.int32, copy=True).reshape(-1)
    dt = _host(dst_tags).astype(np.int32, copy=True).reshape(-1)
    thr = np.full((m,), np.nan, np.float32)
    known = np.zeros((max(int(st.max()) if n else 0, int(dt.max()) if m else 0, 0) + 2,), bool)
    for tag, v in distance_threshold.items():
        if 0 <= int(tag) < known.size:
            known[int(tag)] = True
        thr[dt == int(tag)] = float(v)
    st[(st < 0) | ~known[np.clip(st, 0, None)]] = -1
    dt[(dt < 0) | ~known[np.clip(dt, 0, None)]] = -1
    # the score order: a stable descending sort ON THE DEVICE (equal scores in index order, as numpy's stable argsort of the
    # negated scores gives them; 20 k scores: 1 ms of numpy on the host against ~50 us) -- the scores ride in the one buffer
    sc = _host(src_scores).astype(np.float32).reshape(-1)
    with torch.cuda.device(dev):
        sc, st, dt, thr = _lib.ship(dev, sc, st, dt, thr)
        order = torch.sort(sc, descending=True, stable=True).indices
        src_match = torch.empty((n,), dtype=torch.int32, device=dev)
        dst_match = torch.empty((m,), dtype=torch.int32, device=dev)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.d3d_score_match_workspace_bytes(n, m), dev)
        rc = lib.d3d_score_match(_lib.ptr(distance.contiguous()), n, m, _lib.ptr(st), _lib.ptr(dt), _lib.ptr(thr), _lib.ptr(order),
                                 _lib.ptr(src_match), _lib.ptr(dst_match), _lib.ptr(status), _lib.ptr(ws), ws.numel(),
                                 _lib.stream_ptr())
        _lib.check(rc, "score_match")
    return src_match, dst_match


def score_match_reference_compat(distance, src_scores, src_tags, dst_tags, distance_threshold, src_subset, dst_subset):
    """ScoreMatcher.match exactly as matcher.pyx:142-162 pairs the two orders -- INCLUDING its row mix-up: the k-th best source
    (`src_subset[src_order[k]]`, :157) walks the destinations in the distance order of the k-th row OF THE SUBSET
    (`dst_order[src_idx, ...]` with src_idx the loop counter, :158), i.e. of another box whenever the subset is not already
    sorted by score, and takes the first one that is free, of its tag and within the threshold (match_by_order :96-115 skips a
    failing pair and goes on).  `score_match` walks the source's OWN row -- nearest first -- which is what the docstring of the
    reference's class describes.
    On the device (round 6; a sequential loop of tensor operations before): slot k's acceptable destinations are those of the
    k-th best source (its tag, ITS distance within the threshold, :103-112), their order is that of row k of the subset -- so the
    matrix P[k, j] = distance[subset row k, j] where (k-th best source, j) is acceptable, +inf elsewhere, handed to
    d3d_score_match with the slots in order, reproduces the loop: every slot takes its smallest free entry.
    The score order is the reference's own call on the same values, np.flip(np.argsort(scores)) on the host (so equal scores
    come out as they do there); equal DISTANCES go to the destination earlier in `dst_subset` (np.argsort's unstable default
    leaves that open in the reference); a destination tag missing from `distance_threshold` gets the threshold 0.0, as
    unordered_map::operator[] hands out (:112).
    Returns (src_match[n], dst_match[m]) int32 tensors, -1 = unmatched."""
    return ReferenceAssociation(distance, src_scores, src_tags, dst_tags, distance_threshold, dst_subset).match(src_subset)


_BATCH_MAX_ROWS = 1 << 21              # stacked rows of one batched call (its candidate lists: 512 B of workspace per row)


def _index_array(subset):
    return np.asarray(subset if isinstance(subset, np.ndarray) else list(subset), dtype=np.int64).reshape(-1)


class ReferenceAssociation:
    """score_match_reference_compat for MANY source subsets against one destination subset (the evaluator: 40 score thresholds,
    benchmarks.pyx:218-238): what does not depend on the sources' subset is prepared once -- the destinations' columns of the
    distance matrix, and for every (source, destination) whether the pair is acceptable (tag, the source's OWN distance within the
    destination tag's threshold) -- and `match` queues its work on the stream without reading anything back: the caller
    synchronises once, when it fetches the results."""

    def __init__(self, distance, src_scores, src_tags, dst_tags, distance_threshold, dst_subset):
        self.dev = dev = distance.device
        self.n, self.m = distance.shape
        self.scores = _host(src_scores).astype(np.float32).reshape(-1)
        stags, dtags = _host(src_tags).astype(np.int64).reshape(-1), _host(dst_tags).astype(np.int64).reshape(-1)
        self.dsub = dsub = _index_array(dst_subset)
        if dsub.size == 0 or self.n == 0:
            return
        dt_sub = dtags[dsub]
        thr = _threshold_of(distance_threshold, dt_sub)
        with torch.cuda.device(dev):
            self.dsub_t = torch.from_numpy(dsub).to(dev)
            self.cols = distance.index_select(1, self.dsub_t)                                   # [n, md]
            self.ok = (self.cols <= torch.from_numpy(thr).to(dev)[None, :]) & \
                      (torch.from_numpy(stags).to(dev)[:, None] == torch.from_numpy(dt_sub).to(dev)[None, :])
            md = dsub.size
            self._dtag0 = torch.zeros((md,), dtype=torch.int32, device=dev)
            self._dthr = torch.full((md,), 3.0e38, dtype=torch.float32, device=dev)
            self._inf = torch.full((), float("inf"), dtype=self.cols.dtype, device=dev)
            self._ok_u8 = self.ok.view(torch.uint8)

    def match(self, src_subset):
        """-> (src_match[n], dst_match[m]) int32 tensors on the device, -1 = unmatched (nothing is read back here)"""
        dev, n, m = self.dev, self.n, self.m
        src_match, dst_match = _unmatched(dev, n, m)
        ssub = _index_array(src_subset)
        if ssub.size == 0 or self.dsub.size == 0:
            return src_match, dst_match
        # matcher.pyx:145-146: np.flip(np.argsort([scores of the subset])) -- the same call on the same float64 values (a Python
        # list of floats becomes a float64 array), so equal scores come out as they do there
        src_order = np.flip(np.argsort(self.scores[ssub].astype(np.float64)))
        best = ssub[src_order]                                                                # slot k's source
        lib = _lib.load()
        k, md = int(ssub.size), int(self.dsub.size)
        with torch.cuda.device(dev):
            ssub_t, best_t = _lib.ship(dev, ssub, best)
            # P[k, j] = distance[subset row k, j] where (k-th best source, j) is acceptable, +inf elsewhere
            pref = torch.where(self.ok.index_select(0, best_t), self.cols.index_select(0, ssub_t), self._inf)
            sm = torch.empty((k,), dtype=torch.int32, device=dev)
            dm = torch.empty((md,), dtype=torch.int32, device=dev)
            status = torch.zeros((1,), dtype=torch.int32, device=dev)
            order = torch.arange(k, dtype=torch.int64, device=dev)                            # the slots are in order already
            stag0 = torch.zeros((k,), dtype=torch.int32, device=dev)
            ws = _lib.workspace(lib.d3d_score_match_workspace_bytes(k, md), dev)
            rc = lib.d3d_score_match(_lib.ptr(pref), k, md, _lib.ptr(stag0), _lib.ptr(self._dtag0), _lib.ptr(self._dthr), _lib.ptr(order),
                                     _lib.ptr(sm), _lib.ptr(dm), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            _lib.check(rc, "score_match")
            neg = torch.full((), -1, dtype=torch.int32, device=dev)
            src_match[best_t] = torch.where(sm >= 0, self.dsub_t[sm.clamp_min(0).long()].to(torch.int32), neg)
            dst_match[self.dsub_t] = torch.where(dm >= 0, best_t[dm.clamp_min(0).long()].to(torch.int32), neg)
        return src_match, dst_match


    def match_many(self, src_subsets):
        """`match` for a list of source subsets -> (src_match[T, n], dst_match[T, m]) int32 tensors on the device, row t = the
        association of src_subsets[t].  ONE d3d_score_match_batched call (a few above _BATCH_MAX_ROWS stacked rows): the problems'
        rows stacked, and no stacked matrix -- slot k of a problem reads its distances from the k-th subset row of the prepared
        columns and its acceptable pairs from the k-th best source's row of the prepared mask, by index."""
        dev, n, m = self.dev, self.n, self.m
        T = len(src_subsets)
        src_all, dst_all = _unmatched(dev, n, m, batch=(T,))
        md = int(self.dsub.size)
        if md == 0 or n == 0:
            return src_all, dst_all
        subs = [_index_array(x) for x in src_subsets]
        lib = _lib.load()
        t0 = 0
        while t0 < T:
            t1, rows = t0, 0
            while t1 < T and (t1 == t0 or rows + subs[t1].size <= _BATCH_MAX_ROWS):
                rows += subs[t1].size
                t1 += 1
            if rows == 0:
                t0 = t1
                continue
            B = t1 - t0
            bests = [ss[np.flip(np.argsort(self.scores[ss].astype(np.float64)))] for ss in subs[t0:t1]]      # matcher.pyx:145-146 per subset
            sizes = [ss.size for ss in subs[t0:t1]]
            off = np.zeros((B + 1,), np.int64)
            off[1:] = np.cumsum(sizes)
            local = np.concatenate([np.arange(k, dtype=np.int64) for k in sizes])
            bid = np.repeat(np.arange(B, dtype=np.int64), sizes)
            with torch.cuda.device(dev):
                ssub_t, best_t, off_t, order_t, bid_t = _lib.ship(dev, np.concatenate(subs[t0:t1]), np.concatenate(bests), off, local, bid)
                sm = torch.empty((rows,), dtype=torch.int32, device=dev)
                dm = torch.empty((B, md), dtype=torch.int32, device=dev)
                status = torch.zeros((1,), dtype=torch.int32, device=dev)
                stag0 = torch.zeros((rows,), dtype=torch.int32, device=dev)
                ws = _lib.workspace(lib.d3d_score_match_batched_workspace_bytes(rows, md, B), dev)
                # P[k, j] = cols[subset row k, j] where ok[k-th best source, j], +inf elsewhere -- read through the two index arrays
                rc = lib.d3d_score_match_batched(_lib.ptr(self.cols), _lib.ptr(ssub_t), _lib.ptr(self._ok_u8), _lib.ptr(best_t),
                                                 _lib.ptr(off_t), B, rows, md, _lib.ptr(stag0), _lib.ptr(self._dtag0),
                                                 _lib.ptr(self._dthr), _lib.ptr(order_t), _lib.ptr(sm), _lib.ptr(dm), _lib.ptr(status),
                                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
                _lib.check(rc, "score_match_batched")
                neg = torch.full((), -1, dtype=torch.int32, device=dev)
                # slot k of problem b matched destination slot sm: source best[k] <-> destination dsub[sm]
                src_all[t0:t1][bid_t, best_t] = torch.where(sm >= 0, self.dsub_t[sm.clamp_min(0).long()].to(torch.int32), neg)
                who = best_t[(dm.clamp_min(0).long() + off_t[:B, None]).clamp_max(rows - 1)].to(torch.int32)
                dst_all[t0:t1, self.dsub_t] = torch.where(dm >= 0, who, neg)
            t0 = t1
        return src_all, dst_all


class _BaseMatcher:
    """BaseMatcher's array-level state (matcher.pyx:12-136): the boxes, their distance cache and the two assignment maps"""

    def __init__(self):
        self._cache = None
        self._src = self._dst = None
        self._src_assignment, self._dst_assignment = {}, {}

    def clear_match(self):
        self._src_assignment, self._dst_assignment = {}, {}

    def prepare_boxes(self, src_arr, dst_arr, distance_metric):
        self.clear_match()
        self._src, self._dst = _boxes(src_arr, "src_boxes"), _boxes(dst_arr, "dst_boxes")
        if len(self._src) == 0 or len(self._dst) == 0:
            self._cache = torch.zeros((len(self._src), len(self._dst)), dtype=torch.float32)      # matcher.pyx:41-43
            return
        self._cache = prepare_boxes(self._src, self._dst, distance_metric)

    @property
    def distance_cache(self):
        return self._cache

    def query_src_match(self, src_idx):
        return self._src_assignment.get(int(src_idx), -1)

    def query_dst_match(self, dst_idx):
        return self._dst_assignment.get(int(dst_idx), -1)

    def num_of_matches(self):
        return len(self._src_assignment)


class ScoreMatcher(_BaseMatcher):
    """array-level ScoreMatcher (matcher.pyx:138-162): prepare_boxes, match on subsets, query_* -- same call sequence as the
    reference's evaluator uses (benchmarks.pyx:188-238).  The default reproduces the reference's results: its pairing of the
    k-th best source with the k-th subset row's distance order (matcher.pyx:155-158);
    `reference_compat=False` pairs every source with its own nearest destinations (what the class docstring describes)."""

    def __init__(self, reference_compat=True):
        super().__init__()
        self.reference_compat = bool(reference_compat)

    def match(self, src_subset, dst_subset, distance_threshold):
        self.clear_match()
        src_subset, dst_subset = list(src_subset), list(dst_subset)
        if not src_subset or not dst_subset or self._cache.numel() == 0:
            return
        n, m = self._cache.shape
        stags = np.full((n,), -1, np.int64)
        dtags = np.full((m,), -1, np.int64)
        stags[src_subset] = self._src[src_subset, 0].cpu().numpy().astype(np.int64)
        dtags[dst_subset] = self._dst[dst_subset, 0].cpu().numpy().astype(np.int64)
        if self.reference_compat:
            sm, dm = score_match_reference_compat(self._cache, self._src[:, 1].cpu().numpy(), stags, dtags, distance_threshold,
                                                  src_subset, dst_subset)
        else:      # (boxes outside the subsets carry the tag -1 and take no part)
            sm, dm = score_match(self._cache, self._src[:, 1].cpu().numpy(), stags, dtags, distance_threshold)
        sm, dm = sm.cpu().numpy(), dm.cpu().numpy()
        self._src_assignment = {int(i): int(j) for i, j in enumerate(sm) if j >= 0}
        self._dst_assignment = {int(j): int(i) for j, i in enumerate(dm) if i >= 0}


# ------------------------------------------------------------------------------------------ LSAP, Hungarian, nearest neighbour
LSAP_INVALID, LSAP_INFEASIBLE, LSAP_TOO_BIG = 1, 2, 4          # status bits of d3d_lsap_batched (include/d3d_hip.h)


def _lsap_launch(cost, ld, row_idx, col_idx, row_off, col_off, max_rows, max_cols, dev):
    """one d3d_lsap_batched call; row_idx / col_idx / row_off / col_off int64 numpy arrays, shipped in ONE copy.
    -> (row_match, col_match, status) device tensors (nothing is read back)"""
    lib = _lib.load()
    B = row_off.size - 1
    nrt, nct = int(row_off[-1]), int(col_off[-1])
    with torch.cuda.device(dev):
        ri, ci, ro, co = _lib.ship(dev, row_idx, col_idx, row_off, col_off)
        row_match = torch.empty((nrt,), dtype=torch.int32, device=dev)
        col_match = torch.empty((nct,), dtype=torch.int32, device=dev)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.d3d_lsap_batched_workspace_bytes(B, nrt, nct), dev)
        rc = lib.d3d_lsap_batched(_lib.ptr(cost), _lib.F64 if cost.dtype == torch.float64 else _lib.F32, int(ld), _lib.ptr(ri),
                                  _lib.ptr(ci), _lib.ptr(ro), _lib.ptr(co), B, int(max_rows), int(max_cols), _lib.ptr(row_match),
                                  _lib.ptr(col_match), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "lsap_batched")
    return row_match, col_match, status


def _lsap_raise(status):
    s = int(status)
    if s & LSAP_INVALID:
        raise ValueError("matrix contains invalid numeric entries")
    if s & LSAP_INFEASIBLE:
        raise ValueError("cost matrix is infeasible")
    if s & LSAP_TOO_BIG:
        raise RuntimeError("lsap_batched: a problem beyond the stated sizes or the workspace")


def linear_sum_assignment(cost):
    """scipy.optimize.linear_sum_assignment(cost) on the GPU, the same result bit for bit (ties included): the solver is scipy's
    (Crouse's shortest augmenting path, fp64) step for step.  `cost` is a 2-D matrix -> (row_ind, col_ind), or a [B, n, m] batch
    solved in ONE launch -> (row_ind[B, k], col_ind[B, k]), k = min(n, m).  Accepts numpy arrays (-> int64 numpy arrays, as
    scipy), host tensors (-> int64 host tensors) and device tensors (-> int64 device tensors).  fp32 and fp64 are read as they
    are, other dtypes are widened to fp64 first (as scipy does).  NaN or -inf entries, or a matrix without a full assignment of
    finite cost, raise ValueError (scipy's messages); the call reads its status word back for that."""
    as_numpy = not isinstance(cost, torch.Tensor)
    t = torch.from_numpy(np.asarray(cost)) if as_numpy else cost.detach()
    if t.dim() not in (2, 3):
        raise ValueError("expected a matrix (2-D array) or a batch of matrices (3-D array), got shape %r" % (tuple(t.shape),))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    odev = t.device
    batched = t.dim() == 3
    if not batched:
        t = t[None]
    B, n, m = t.shape
    k = min(n, m)
    if B == 0 or k == 0:
        empty = torch.zeros((B, 0) if batched else (0,), dtype=torch.int64)
        return (empty.numpy(), empty.numpy()) if as_numpy else (empty.to(odev), empty.to(odev))
    dev = device_of(t)
    c = t.to(dev).contiguous().view(B * n, m)
    row_idx = np.arange(B * n, dtype=np.int64)
    col_idx = np.tile(np.arange(m, dtype=np.int64), B)
    row_match, col_match, status = _lsap_launch(c, m, row_idx, col_idx, np.arange(B + 1, dtype=np.int64) * n,
                                                np.arange(B + 1, dtype=np.int64) * m, n, m, dev)
    with torch.cuda.device(dev):
        if n <= m:              # every row is assigned: scipy returns rows 0 .. n-1 in order
            rows = torch.arange(n, dtype=torch.int64, device=dev).expand(B, n)
            cols = row_match.view(B, n).to(torch.int64)
        else:                   # every column is assigned: scipy orders the pairs by row
            cm = col_match.view(B, m).to(torch.int64)
            order = torch.argsort(cm, dim=1)
            rows, cols = torch.gather(cm, 1, order), order
        st = status.cpu()
    _lsap_raise(st[0])
    if not batched:
        rows, cols = rows[0], cols[0]
    if as_numpy:
        return rows.cpu().numpy(), cols.cpu().numpy()
    return _lib.to_caller((rows.contiguous(), cols.contiguous()), odev, dev)


def _matrix_on_device(distance):
    t = torch.from_numpy(np.ascontiguousarray(distance, dtype=np.float32)) if not isinstance(distance, torch.Tensor) else distance
    if t.dim() != 2:
        raise ValueError("distance should be a [n, m] matrix")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    dev = device_of(t)
    return t.to(dev).contiguous(), dev


def _tags(tags, count, what):
    t = _host(tags).reshape(-1)
    if t.size != count:
        raise ValueError("%s should hold one tag per box (%d), got %d" % (what, count, t.size))
    return t.astype(np.int64)


def _subset(subset, count, what):
    s = np.arange(count, dtype=np.int64) if subset is None else _index_array(_host(subset) if isinstance(subset, torch.Tensor) else subset)
    if s.size and (s.min() < 0 or s.max() >= count):
        raise ValueError("%s holds an index outside 0 .. %d" % (what, count - 1))
    return s


def _hungarian_problems(stags, dtags, ssub, dsub):
    """HungarianMatcher.match's split (matcher.pyx:194-220): the subsets by class, subset order kept inside each class, the
    classes in first-appearance order among the sources, those without destinations skipped.  -> (row lists, column lists)"""
    rows, cols = {}, {}
    for s in ssub.tolist():
        rows.setdefault(int(stags[s]), []).append(s)
    for d in dsub.tolist():
        cols.setdefault(int(dtags[d]), []).append(d)
    keep = [c for c in rows if c in cols]
    return [rows[c] for c in keep], [cols[c] for c in keep], keep


def hungarian_match(distance, src_tags, dst_tags, distance_threshold, src_subset=None, dst_subset=None):
    """HungarianMatcher.match (matcher.pyx:188-230) on arrays: per class, the optimal assignment of
    distance[src of the class, dst of the class] (scipy's linear_sum_assignment, reproduced bit for bit, ties included), then
    the pairs with distance <= distance_threshold[class] (0.0 for a class missing from the map) are kept -- the assignment is not
    solved again without the others.  All classes in ONE launch.  `distance` f32 [n, m] (a device tensor, or moved there),
    tags one per box, subsets default to every box.  -> (src_match[n], dst_match[m]) int32 device tensors, -1 = unmatched.
    A NaN or -inf distance inside a class's block raises ValueError, as scipy does (the call reads its status word back)."""
    dist, dev = _matrix_on_device(distance)
    n, m = dist.shape
    stags, dtags = _tags(src_tags, n, "src_tags"), _tags(dst_tags, m, "dst_tags")
    ssub, dsub = _subset(src_subset, n, "src_subset"), _subset(dst_subset, m, "dst_subset")
    src_match, dst_match = _unmatched(dev, n, m)
    rows, cols, classes = _hungarian_problems(stags, dtags, ssub, dsub)
    if not rows:
        return src_match, dst_match
    nr = np.array([len(r) for r in rows], np.int64)
    nc = np.array([len(c) for c in cols], np.int64)
    row_off, col_off = np.zeros((len(rows) + 1,), np.int64), np.zeros((len(rows) + 1,), np.int64)
    row_off[1:], col_off[1:] = np.cumsum(nr), np.cumsum(nc)
    row_idx, col_idx = np.concatenate([np.asarray(r, np.int64) for r in rows]), np.concatenate([np.asarray(c, np.int64) for c in cols])
    thr = np.repeat(_threshold_of(distance_threshold, np.asarray(classes, np.int64)), nr)        # (one class per problem)
    row_match, _, status = _lsap_launch(dist, m, row_idx, col_idx, row_off, col_off, int(nr.max()), int(nc.max()), dev)
    with torch.cuda.device(dev):
        ri, cbase, thr_t, ci_all = _lib.ship(dev, row_idx, np.repeat(col_off[:-1], nr), thr, col_idx)
        has = row_match >= 0
        cj = ci_all[(cbase + row_match.clamp_min(0).to(torch.int64))]
        ok = has & (dist[ri, cj] <= thr_t)
        src_match[ri[ok]] = cj[ok].to(torch.int32)
        dst_match[cj[ok]] = ri[ok].to(torch.int32)
        st = status.cpu()
    _lsap_raise(st[0])
    return src_match, dst_match


def nearest_neighbor_match(distance, src_tags, dst_tags, distance_threshold, src_subset=None, dst_subset=None, src_free=None,
                           dst_free=None):
    """NearestNeighborMatcher.match (matcher.pyx:164-186 + match_by_order :90-121) on arrays: the (src, dst) pairs of the two
    subsets from the least distance up; a pair is taken when neither side is taken yet, the tags agree and
    distance <= distance_threshold[dst tag] (0.0 for a tag missing from the map).  Equal distances: row-major order of the
    subset positions (what a stable sort gives; the reference's unstable argsort leaves it open).  src_free[n] / dst_free[m]
    (bool, optional): False = the box was matched by an earlier call and takes no part.  -> (src_match[n], dst_match[m]) int32
    device tensors, -1 = unmatched.  Nothing is read back."""
    dist, dev = _matrix_on_device(distance)
    n, m = dist.shape
    stags, dtags = _tags(src_tags, n, "src_tags"), _tags(dst_tags, m, "dst_tags")
    ssub, dsub = _subset(src_subset, n, "src_subset"), _subset(dst_subset, m, "dst_subset")
    src_match, dst_match = _unmatched(dev, n, m)
    ns, nd = ssub.size, dsub.size
    if ns == 0 or nd == 0:
        return src_match, dst_match
    lib = _lib.load()
    st, dt = stags[ssub].astype(np.int32), dtags[dsub].astype(np.int32)
    thr = _threshold_of(distance_threshold, dt)
    sf = np.ones((ns,), np.uint8) if src_free is None else _host(src_free).reshape(-1).astype(bool)[ssub].astype(np.uint8)
    df = np.ones((nd,), np.uint8) if dst_free is None else _host(dst_free).reshape(-1).astype(bool)[dsub].astype(np.uint8)
    with torch.cuda.device(dev):
        si, di, st_t, dt_t, thr_t, sf_t, df_t = _lib.ship(dev, ssub, dsub, st, dt, thr, sf, df)      # (one copy)
        sm = torch.empty((ns,), dtype=torch.int32, device=dev)
        dm = torch.empty((nd,), dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.d3d_nn_match_workspace_bytes(ns, nd), dev)
        rc = lib.d3d_nn_match(_lib.ptr(dist), m, _lib.ptr(si), ns, _lib.ptr(di), nd, _lib.ptr(st_t), _lib.ptr(dt_t), _lib.ptr(thr_t),
                              _lib.ptr(sf_t), _lib.ptr(df_t), _lib.ptr(sm), _lib.ptr(dm), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "nn_match")
        hs, hd = sm >= 0, dm >= 0
        src_match[si[hs]] = di[sm[hs].to(torch.int64)].to(torch.int32)
        dst_match[di[hd]] = si[dm[hd].to(torch.int64)].to(torch.int32)
    return src_match, dst_match


class _AssignmentMatcher(_BaseMatcher):
    """the base of the two matchers below.  Unlike ScoreMatcher here, `match` does not clear the assignment first -- as in the
    reference, a second `match` without clear_match / prepare_boxes adds to it --, so the two maps are
    checked against each other when they are counted."""

    def _tags(self):
        return self._src[:, 0].cpu().numpy().astype(np.int64), self._dst[:, 0].cpu().numpy().astype(np.int64)

    def num_of_matches(self):
        assert len(self._src_assignment) == len(self._dst_assignment)
        return super().num_of_matches()


class NearestNeighborMatcher(_AssignmentMatcher):
    """NearestNeighborMatcher (matcher.pyx:164-186): the pairs from the closest up (nearest_neighbor_match); boxes that an
    earlier `match` assigned take no part."""

    def match(self, src_subset, dst_subset, distance_threshold):
        src_subset, dst_subset = list(src_subset), list(dst_subset)
        if not src_subset or not dst_subset or self._cache is None or self._cache.numel() == 0:
            return
        n, m = self._cache.shape
        stags, dtags = self._tags()
        sf, df = np.ones((n,), bool), np.ones((m,), bool)
        sf[list(self._src_assignment)] = False
        df[list(self._dst_assignment)] = False
        sm, dm = nearest_neighbor_match(self._cache, stags, dtags, distance_threshold, src_subset, dst_subset, sf, df)
        sm = sm.cpu().numpy()
        for i in np.nonzero(sm >= 0)[0].tolist():
            self._src_assignment[i] = int(sm[i])
            self._dst_assignment[int(sm[i])] = i


class HungarianMatcher(_AssignmentMatcher):
    """HungarianMatcher (matcher.pyx:188-230): the optimal assignment per class (hungarian_match, every class in one launch);
    a second `match` overwrites the assignment key by key, as the reference's maps do."""

    def match(self, src_subset, dst_subset, distance_threshold):
        src_subset, dst_subset = list(src_subset), list(dst_subset)
        if not src_subset or not dst_subset or self._cache is None or self._cache.numel() == 0:
            return
        stags, dtags = self._tags()
        sm, _ = hungarian_match(self._cache, stags, dtags, distance_threshold, src_subset, dst_subset)
        sm = sm.cpu().numpy()
        for i in np.nonzero(sm >= 0)[0].tolist():
            self._src_assignment[i] = int(sm[i])
            self._dst_assignment[int(sm[i])] = i
