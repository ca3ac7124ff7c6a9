"""Numpy models of the centre-head operators (include/d3d_hip.h, csrc/center.hip): heatmap_peaks, circle_nms, gaussian_heatmap.
Each follows the rule in the header literally; test_center.py checks them against independent formulations (torch's max_pool2d and
topk, a distance-matrix sweep, CenterNet's float gaussian2D), test_gpu_center.py checks the kernels against them."""
import numpy as np


def desc_key(v):
    """KeyBits<K>::desc of csrc/lds_sort.hpp for a float32 / float64 array: unsigned keys whose ASCENDING order is descending value,
    -0 == +0, every NaN first"""
    v = np.ascontiguousarray(v)
    u, top = (np.uint32, np.uint32(1 << 31)) if v.dtype == np.float32 else (np.uint64, np.uint64(1 << 63))
    b = v.view(u).copy()
    b[b == top] = 0                                           # -0 -> +0
    asc = np.where(b & top, ~b, b | top)
    key = ~asc
    key[np.isnan(v)] = 0
    return key


def peak_mask(heat, kernel):
    """heat [B, C, H, W] float32 -> bool: no NaN in the kernel x kernel window (clipped to the plane) and the value >= every value of
    it.  A literal loop over the window's offsets; a comparison with a NaN on either side is False."""
    r = kernel // 2
    h, w = heat.shape[2:]
    ok = ~np.isnan(heat)
    with np.errstate(invalid="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))          # cells whose neighbour exists
                yn, xn = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                ok[:, :, ys, xs] &= heat[:, :, ys, xs] >= heat[:, :, yn, xn]
    return ok


def heatmap_peaks_model(heat, k, kernel=3, threshold=None):
    """heat [B, C, H, W] float32 (a half-precision map widened exactly) -> (flat [B, k] int64: the flat index (c * H + y) * W + x of
    every rank, -1 for a missing slot; counts [B] int32).  Candidates = peaks with value > float32(threshold); a stable sort on
    (key, flat index)."""
    heat = np.ascontiguousarray(heat, np.float32)
    b = heat.shape[0]
    cand = peak_mask(heat, kernel)
    if threshold is not None:
        with np.errstate(invalid="ignore"):
            cand &= heat > np.float32(threshold)
    flat = np.full((b, k), -1, np.int64)
    counts = np.zeros((b,), np.int32)
    for s in range(b):
        idx = np.flatnonzero(cand[s].reshape(-1))
        key = desc_key(heat[s].reshape(-1)[idx])
        order = np.lexsort((idx, key))[:k]                    # key first, then the flat index
        counts[s] = len(order)
        flat[s, :len(order)] = idx[order]
    return flat, counts


def unravel_peaks(flat, shape):
    """flat [B, k] -> (classes, ys, xs) int32, -1 where flat is -1"""
    _, _, h, w = shape
    miss = flat < 0
    f = np.where(miss, 0, flat)
    out = [f // (h * w), f % (h * w) // w, f % w]
    return tuple(np.where(miss, -1, o).astype(np.int32) for o in out)


def argsort_desc_model(scores):
    """argsort_desc's order: descending score, NaN first, ties in ascending row"""
    return np.lexsort((np.arange(len(scores)), desc_key(scores)))


def _cap(keep, visited, max_keep):
    if max_keep is not None:
        kept = [i for i in visited if keep[i]]
        keep[np.asarray(kept[max_keep:], np.int64)] = False


def circle_nms_model(centers, scores, dist2_threshold, offsets=None, max_keep=None):
    """det3d's circle_nms loop in the dtype of `centers`, inside every segment [offsets[s], offsets[s + 1]) -> keep bool[N]"""
    n = len(centers)
    dtype = centers.dtype.type
    x, y = np.ascontiguousarray(centers[:, 0]), np.ascontiguousarray(centers[:, 1])
    t = dtype(dist2_threshold)
    offsets = [0, n] if offsets is None else list(offsets)
    keep = np.zeros((n,), bool)
    for lo, hi in zip(offsets, offsets[1:]):
        order = lo + argsort_desc_model(scores[lo:hi])
        sup = np.zeros((n,), bool)
        for a, i in enumerate(order):
            if sup[i]:
                continue
            keep[i] = True
            later = order[a + 1:]                             # (the loop over the later rows, all at once)
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy = x[i] - x[later], y[i] - y[later]     # arrays of the dtype: one rounding per operation
                sup[later[dx * dx + dy * dy <= t]] = True
        _cap(keep, order, max_keep)
    return keep


def circle_nms_matrix(centers, scores, dist2_threshold, offsets=None, max_keep=None):
    """the same rule a second way: the full d2 matrix of a segment in its visiting order, then a sequential sweep over its rows"""
    n = len(centers)
    t = centers.dtype.type(dist2_threshold)
    offsets = [0, n] if offsets is None else list(offsets)
    keep = np.zeros((n,), bool)
    for lo, hi in zip(offsets, offsets[1:]):
        order = lo + argsort_desc_model(scores[lo:hi])
        x, y = centers[order, 0], centers[order, 1]
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
            hit = np.triu((dx * dx + dy * dy) <= t, 1)        # row suppresses LATER ranks only; NaN <= t is False
        alive = np.ones((len(order),), bool)
        for a in range(len(order)):
            if alive[a]:
                alive &= ~hit[a]
        keep[order] = alive
        _cap(keep, order, max_keep)
    return keep


def gaussian_heatmap_model(centers, radii, classes, shape, offsets=None):
    """the per-box loop: np.maximum of the map's clipped slice with float32(exp(-(double)(18 d2) / (double)((2 r + 1)^2)))"""
    b, c, h, w = shape
    out = np.zeros(shape, np.float32)
    offsets = [0, len(centers)] if offsets is None else list(offsets)
    for s in range(b):
        for i in range(offsets[s], offsets[s + 1]):
            cx, cy, r = int(centers[i, 0]), int(centers[i, 1]), int(radii[i])
            x0, x1, y0, y1 = max(cx - r, 0), min(cx + r, w - 1), max(cy - r, 0), min(cy + r, h - 1)
            if x0 > x1 or y0 > y1:
                continue
            yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
            d2 = (xx - cx) ** 2 + (yy - cy) ** 2
            g = np.exp(-(18 * d2).astype(np.float64) / np.float64((2 * r + 1) * (2 * r + 1))).astype(np.float32)
            view = out[s, int(classes[i]), y0:y1 + 1, x0:x1 + 1]
            np.maximum(view, g, out=view)
    return out


def ulp_distance(a, b):
    """the distance of two float32 arrays of finite, non-negative values in units in the last place"""
    return np.abs(np.ascontiguousarray(a).view(np.int32).astype(np.int64) - np.ascontiguousarray(b).view(np.int32).astype(np.int64))
