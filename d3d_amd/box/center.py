"""d3d_amd.box.center -- the centre head of CenterPoint / BEVFusion / BEVDet / OpenPCDet's CenterHead: what stands between the BEV
map and box2d_nms.  An extension (the reference has no counterpart).

    target = gaussian_heatmap(centers, gaussian_radius(w, l), classes, (B, C, H, W), offsets)      # training: the target map
    peaks = heatmap_peaks(heat, k=500, kernel=3)                                                   # inference: the K best local maxima
    reg = gather_at_peaks(regression_maps, peaks)                                                  # [B, k, C'] at the peaks
    keep = circle_nms(xy, scores, dist2_threshold, offsets=offsets, max_keep=83)                   # CenterPoint's circle NMS

Defined exactly (the rules: include/d3d_hip.h; kernels: csrc/center.hip): integers, copies of input bits and one rounded expression --
no float atomics, the same bits on every run, nothing read back inside a call.  Every refusal raises before a GPU is needed.
"""
import collections

import numpy as np
import torch

from .. import _lib
from .._rows import FLOAT_CODES, as_tensor, device_of, dtype_code, group_ids, host_offsets, rows_on

PEAK_CODES = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
_PEAK_K_MAX = 4096                  # d3d_heatmap_peaks_max()
_CIRCLE_MAX = 4096                  # d3d_circle_nms_max()
_RADIUS_MAX = 4095
_INT_MAX = 2 ** 31 - 1
_GRID_MAX = 65535                   # samples (and, drawing, classes) of one call: a launch grid's second and third extent
_DRAW_SIDE_MAX = 2 ** 30

HeatmapPeaks = collections.namedtuple("HeatmapPeaks", "scores classes ys xs counts")


def heatmap_peaks_max():
    """The largest k of heatmap_peaks.  Pure host."""
    return int(_lib.load().d3d_heatmap_peaks_max())


def circle_nms_max():
    """The longest segment circle_nms takes.  Pure host."""
    return int(_lib.load().d3d_circle_nms_max())


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _egress(tensors, odev, dev, was_numpy):
    out = _lib.to_caller(tuple(tensors), odev, dev)
    return tuple(t.numpy() for t in out) if was_numpy else out


def heatmap_peaks(heat, k, kernel=3, threshold=None):
    """The k best local maxima of every sample of a heat map: CenterNet's max_pool2d + `==` + topk (OpenPCDet: two topk's) in one call.

    :param heat: [B, C, H, W] float32, float16 or bfloat16; torch tensor (GPU or host) or numpy array, any strides (made contiguous);
        C * H * W <= 2^31 - 1, B <= 65535.  Only read
    :param k: 1 .. heatmap_peaks_max() (4096)
    :param kernel: 1, 3, 5 or 7.  A cell is a PEAK iff no value of its kernel x kernel window (clipped to the plane, inside its own
        class plane) is NaN and its value is >= every value of the window: exactly max_pool2d(heat, kernel, 1, kernel // 2) == heat.
        kernel=1: every cell that is not NaN (a plain top-k).  -0.0 == +0.0; every cell of a plateau is a peak
    :param threshold: None, or a float (rounded to float32): only peaks whose value (widened to float32) is > threshold count
    :return: HeatmapPeaks(scores [B, k] in heat's dtype, classes, ys, xs [B, k] int32, counts [B] int32) on the side heat came from.
        Ranked by descending value (equal values, and -0 against +0, are ties), ties to the lowest flat index (c * H + y) * W + x --
        not torch.topk's unspecified tie order.  scores holds the input's own bits; missing slots are -inf / -1;
        counts = min(k, candidates)

    No sigmoid inside: sigmoid is monotone, apply it to the [B, k] scores.  Peaks and ties are those of the values passed in (two
    logits that differ may have equal sigmoids; here they are not ties).
    """
    heat, was_numpy = as_tensor(heat, "heat")
    if heat.dim() != 4:
        raise ValueError("heat must be [B, C, H, W], not %s" % (tuple(heat.shape),))
    code = dtype_code(heat, PEAK_CODES, "heat")
    if not _is_int(k) or not 1 <= int(k) <= _PEAK_K_MAX:
        raise ValueError("k must be an int in 1 .. %d, not %r" % (_PEAK_K_MAX, k))
    if not _is_int(kernel) or int(kernel) not in (1, 3, 5, 7):
        raise ValueError("kernel must be 1, 3, 5 or 7, not %r" % (kernel,))
    b, c, h, w = heat.shape
    if c < 1 or h < 1 or w < 1:
        raise ValueError("heat has an empty plane: %s" % (tuple(heat.shape),))
    if c * h * w > _INT_MAX or b > _GRID_MAX:
        raise ValueError("heatmap_peaks takes C * H * W <= 2^31 - 1 and B <= %d, not %s" % (_GRID_MAX, tuple(heat.shape)))
    if threshold is not None:
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold is NaN")
    k, kernel = int(k), int(kernel)
    lib = _lib.load()
    dev = device_of(heat)
    with torch.cuda.device(dev):
        x = heat.detach().to(dev).contiguous()
        scores = torch.empty((b, k), dtype=heat.dtype, device=dev)
        classes, ys, xs = (torch.empty((b, k), dtype=torch.int32, device=dev) for _ in range(3))
        counts = torch.empty((b,), dtype=torch.int32, device=dev)
        if b:
            ws = _lib.workspace(lib.d3d_heatmap_peaks_workspace_bytes(b, c, h, w, k), dev)
            rc = lib.d3d_heatmap_peaks(_lib.ptr(x), b, c, h, w, code, k, kernel, int(threshold is not None),
                                       0.0 if threshold is None else threshold, _lib.ptr(scores), _lib.ptr(classes), _lib.ptr(ys),
                                       _lib.ptr(xs), _lib.ptr(counts), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
            _lib.check(rc, "heatmap_peaks")
    return HeatmapPeaks(*_egress((scores, classes, ys, xs, counts), heat.device, dev, was_numpy))


def gather_at_peaks(maps, peaks):
    """The regression maps at the peaks: maps [B, C', H, W] -> [B, k, C'], rows of missing slots zero.  Plain torch indexing (no
    kernel), on maps' device, differentiable in maps.  peaks: a HeatmapPeaks (or anything with ys and xs [B, k], -1 = missing)."""
    maps, was_numpy = as_tensor(maps, "maps")
    if maps.dim() != 4:
        raise ValueError("maps must be [B, C', H, W], not %s" % (tuple(maps.shape),))
    ys = torch.as_tensor(peaks.ys).to(maps.device).long()
    xs = torch.as_tensor(peaks.xs).to(maps.device).long()
    b, c, h, w = maps.shape
    if ys.dim() != 2 or ys.shape != xs.shape or ys.shape[0] != b:
        raise ValueError("peaks of %s do not belong to maps of %s" % (tuple(ys.shape), tuple(maps.shape)))
    present = (ys >= 0) & (xs >= 0)
    flat = torch.where(present, ys * w + xs, torch.zeros_like(ys))
    rows = maps.reshape(b, c, h * w).gather(2, flat[:, None, :].expand(b, c, flat.shape[1])).transpose(1, 2)
    out = torch.where(present[..., None], rows, torch.zeros_like(rows)).contiguous()
    return out.detach().numpy() if was_numpy else out


def _segments_of_groups(groups, n):
    """-> (perm, seg_offsets [G + 1], the longest segment), on the device groups live on: box2d_nms_batched's stable sort"""
    groups = group_ids(groups)
    if groups.dim() != 1 or len(groups) != n:
        raise ValueError("Numbers of centers and groups are inconsistent!")
    ids, perm = torch.sort(groups, stable=True)                # stable: a segment's rows stay in ascending row order
    counts = torch.unique_consecutive(ids, return_counts=True)[1]
    seg = torch.zeros((counts.numel() + 1,), dtype=torch.int64, device=groups.device)
    seg[1:] = counts.cumsum(0)
    return perm, seg, int(counts.max())                        # (the one host read)


def circle_nms(centers, scores, dist2_threshold, offsets=None, groups=None, max_keep=None):
    """CenterPoint's circle NMS (det3d's circle_nms, a numba loop on the host) inside every segment of a batch; returns the KEEP mask
    bool[N] on the side the centers came from.

    :param centers: [N, D], D >= 2, float32 or float64: columns 0 and 1 are (x, y); rows of a wider tensor are read as they lie
    :param scores: [N] in the same dtype
    :param dist2_threshold: the SQUARED distance, rounded to the dtype.  (CenterPoint's configs pass what they call a radius straight
        into this slot: nms.min_radius = [4, 12, 10, ...] are squared distances.)
    :param offsets: host [S + 1] segment boundaries, rows offsets[s] .. offsets[s + 1] form segment s; or
    :param groups: [N] integers of any dtype and any values (negative, with gaps, unsorted): rows with equal values form a segment.
        Both: ValueError; neither: one segment.  A segment holds at most circle_nms_max() (4096) rows -- a detector passes its top-k
    :param max_keep: CenterPoint's post_max_size: only the first max_keep kept rows of a segment, in visiting order, stay True

    Inside a segment the rows are visited in argsort_desc's order: descending score, NaN first, ties in ascending row.  A visited
    row that is not suppressed is kept, and suppresses every later row j with (xi - xj)^2 + (yi - yj)^2 <= dist2_threshold, every
    operation rounded once in the dtype; a NaN distance suppresses nothing, a suppressed row suppresses nothing.  Never across
    segments.  One launch, one workgroup per segment.
    """
    centers, was_numpy = as_tensor(centers, "centers")
    scores, _ = as_tensor(scores, "scores")
    if centers.dim() != 2 or centers.shape[1] < 2:
        raise ValueError("centers must be [N, D] with D >= 2 (columns 0 and 1 are x and y), not %s" % (tuple(centers.shape),))
    code = dtype_code(centers, FLOAT_CODES, "centers")
    if scores.dtype != centers.dtype:
        raise ValueError("centers and scores must have the same dtype, not %s and %s" % (centers.dtype, scores.dtype))
    if scores.dim() != 1 or len(scores) != len(centers):
        raise ValueError("Numbers of centers and scores are inconsistent!")
    if offsets is not None and groups is not None:
        raise ValueError("give offsets or groups, not both")
    if max_keep is not None and (not _is_int(max_keep) or int(max_keep) < 0):
        raise ValueError("max_keep must be None or an int >= 0, not %r" % (max_keep,))
    threshold = float(dist2_threshold)
    n = len(centers)
    perm = None
    if groups is None:
        offs = host_offsets(offsets, n, "offsets")
        seg = torch.tensor(offs, dtype=torch.int64)
        largest = max([hi - lo for lo, hi in zip(offs, offs[1:])], default=0)
    elif n:
        perm, seg, largest = _segments_of_groups(groups, n)
    else:
        if len(groups):
            raise ValueError("Numbers of centers and groups are inconsistent!")
        seg, largest = torch.zeros((1,), dtype=torch.int64), 0
    if largest > _CIRCLE_MAX:
        raise ValueError("a segment of %d rows: circle_nms takes at most %d per segment (pass the top-k)" % (largest, _CIRCLE_MAX))
    if n == 0:
        empty = torch.zeros((0,), dtype=torch.bool)
        return empty.numpy() if was_numpy else empty
    lib = _lib.load()
    dev = device_of(centers, scores)
    with torch.cuda.device(dev):
        c, stride = rows_on(centers, dev)
        s = scores.detach().to(dev).contiguous()
        seg = seg.to(dev)
        perm = None if perm is None else perm.to(dev)
        keep = torch.empty((n,), dtype=torch.uint8, device=dev)
        rc = lib.d3d_circle_nms(_lib.ptr(c), stride, _lib.ptr(s), None if perm is None else _lib.ptr(perm), _lib.ptr(seg), n, seg.numel() - 1,
                                largest, code, threshold, _INT_MAX if max_keep is None else min(int(max_keep), _INT_MAX),
                                _lib.ptr(keep), _lib.stream_ptr())
        _lib.check(rc, "circle_nms")
    return _egress((keep.view(torch.bool),), centers.device, dev, was_numpy)[0]


def _int_rows(x, what, dim):
    t, was_numpy = as_tensor(x, what)
    if t.dim() != dim or t.dtype == torch.bool or t.is_floating_point() or t.is_complex():
        raise ValueError("%s must be a %d-D tensor of integers, not %s of %s" % (what, dim, t.dtype, tuple(t.shape)))
    return t, was_numpy


def gaussian_heatmap(centers, radii, classes, shape, offsets=None):
    """The centre head's target map: every ground-truth box draws a Gaussian into its class plane, overlaps keep the maximum --
    CenterNet's draw_umich_gaussian for all boxes of a batch in one launch (OpenPCDet: a Python loop over boxes).

    :param centers: [M, 2] integers (x, y) = (column, row); anywhere, outside the map too
    :param radii: [M] integers in 0 .. 4095 (gaussian_radius gives them)
    :param classes: [M] integers in [0, C)
    :param shape: (B, C, H, W)
    :param offsets: host [B + 1] boundaries: boxes offsets[b] .. offsets[b + 1] belong to sample b.  None: B == 1
    :return: [B, C, H, W] float32 on the side the centers came from.  out[b, c, y, x] is the maximum of 0 and, over the boxes of
        sample b and class c with |x - cx| <= r and |y - cy| <= r, of float32(exp(-18 * d2 / (2 r + 1)^2)), d2 = (x - cx)^2 + (y - cy)^2:
        gaussian2D with sigma = (2 r + 1) / 6 over the square window, clipped at the borders; integers exact, one float64 division, one
        float64 exp, one rounding.  The centre cell is exactly 1.0.  Every element is written once (zeros too); no atomics
    """
    centers, was_numpy = _int_rows(centers, "centers", 2)
    radii, _ = _int_rows(radii, "radii", 1)
    classes, _ = _int_rows(classes, "classes", 1)
    if centers.shape[1] != 2:
        raise ValueError("centers must be [M, 2] rows (x, y), not %s" % (tuple(centers.shape),))
    m = len(centers)
    if len(radii) != m or len(classes) != m:
        raise ValueError("centers, radii and classes must have one row per box: %d, %d, %d" % (m, len(radii), len(classes)))
    if not isinstance(shape, (tuple, list, torch.Size)) or len(shape) != 4 or not all(_is_int(v) and int(v) >= 0 for v in shape):
        raise ValueError("shape must be (B, C, H, W), not %r" % (shape,))
    b, c, h, w = (int(v) for v in shape)
    if b > _GRID_MAX or c > _GRID_MAX or h > _DRAW_SIDE_MAX or w > _DRAW_SIDE_MAX or m > _INT_MAX:
        raise ValueError("gaussian_heatmap takes B, C <= %d and H, W <= 2^30, not %r" % (_GRID_MAX, tuple(shape)))
    if offsets is None and b != 1:
        raise ValueError("a batch of %d samples needs offsets" % b)
    offs = host_offsets(offsets, m, "offsets")
    if len(offs) != b + 1:
        raise ValueError("offsets names %d samples, shape %d" % (len(offs) - 1, b))
    if m:                                                              # (one read-back each when the boxes live on a GPU)
        if bool(((classes < 0) | (classes >= c)).any()):
            raise ValueError("classes holds values outside [0, %d)" % c)
        if bool(((radii < 0) | (radii > _RADIUS_MAX)).any()):
            raise ValueError("radii holds values outside 0 .. %d" % _RADIUS_MAX)
    lib = _lib.load()
    dev = device_of(centers, radii, classes)
    with torch.cuda.device(dev):
        out = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
        if out.numel():
            # a centre further than 4095 cells outside the map draws nothing: clamped there it fits int32 and still draws nothing
            xy = centers.detach().to(dev).long()
            lo = xy.new_tensor([-_RADIUS_MAX - 1, -_RADIUS_MAX - 1])
            xy = torch.minimum(torch.maximum(xy, lo), xy.new_tensor([w + _RADIUS_MAX, h + _RADIUS_MAX])).int().contiguous()
            r, cl = radii.detach().to(dev).int().contiguous(), classes.detach().to(dev).int().contiguous()
            seg = torch.tensor(offs, dtype=torch.int64).to(dev)
            rc = lib.d3d_gaussian_heatmap(_lib.ptr(xy), _lib.ptr(r), _lib.ptr(cl), _lib.ptr(seg), m, b, c, h, w, _lib.ptr(out),
                                          _lib.stream_ptr())
            _lib.check(rc, "gaussian_heatmap")
    return _egress((out,), centers.device, dev, was_numpy)[0]


def gaussian_radius(footprint_w, footprint_l, min_overlap=0.1, min_radius=2):
    """CenterNet's gaussian_radius (the smallest of the three roots, as CornerNet wrote it and OpenPCDet's centernet_utils keeps it) for
    boxes whose footprint is footprint_w x footprint_l cells; plain tensor arithmetic, no kernel.  Tensors, arrays or numbers in;
    -> an int32 tensor max(int(r), min_radius), on the inputs' device: gaussian_heatmap's radii."""
    w = torch.as_tensor(footprint_w)
    w = w if w.is_floating_point() else w.to(torch.float32)
    l = torch.as_tensor(footprint_l).to(device=w.device, dtype=w.dtype)
    mo = float(min_overlap)
    b1 = l + w
    c1 = w * l * (1 - mo) / (1 + mo)
    r1 = (b1 + torch.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (l + w)
    c2 = (1 - mo) * w * l
    r2 = (b2 + torch.sqrt(b2 * b2 - 16 * c2)) / 2
    a3 = 4 * mo
    b3 = -2 * mo * (l + w)
    c3 = (mo - 1) * w * l
    r3 = (b3 + torch.sqrt(b3 * b3 - 4 * a3 * c3)) / 2
    r = torch.minimum(torch.minimum(r1, r2), r3)
    return torch.clamp_min(r.to(torch.int32), int(min_radius))


__all__ = ["HeatmapPeaks", "heatmap_peaks", "heatmap_peaks_max", "gather_at_peaks", "circle_nms", "circle_nms_max", "gaussian_heatmap",
           "gaussian_radius"]
