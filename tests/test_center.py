"""CPU: the centre-head operators without a GPU -- the numpy models of center_reference.py against independent formulations (torch's
max_pool2d / topk and OpenPCDet's two-stage top-k; a distance-matrix sweep; CenterNet's float gaussian2D), every refusal of the
three fronts before a device is needed, and the C entries' declarations and argument codes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import center_cases as cases
import center_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("d3d_heatmap_peaks", "d3d_heatmap_peaks_workspace_bytes", "d3d_heatmap_peaks_max", "d3d_circle_nms", "d3d_circle_nms_max",
           "d3d_gaussian_heatmap")


def test_entry_points_are_declared_exported_and_bound():
    from d3d_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3d_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, decl), "include/d3d_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libd3d_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    section = src[src.index("the centre head: peaks of a heat map"):]
    assert "never fires" in section and "reference has no counterpart" in section      # the eps mask's note, the provenance
    lib = _lib.load()
    assert lib.d3d_abi_version() == 13
    assert lib.d3d_heatmap_peaks_max() == 4096 and lib.d3d_circle_nms_max() == 4096
    # the workspace is bounded by bins + tiles + k per sample, not by the map: 4 x 10 x 180 x 180 fp32 is 5.2 MB
    small = lib.d3d_heatmap_peaks_workspace_bytes(4, 10, 180, 180, 500)
    assert 4 * 3 * 4096 * 4 < small < 4 * (3 * 4096 * 4 + 320 * 8 + 500 * 8 + 4096)
    assert lib.d3d_heatmap_peaks_workspace_bytes(1, 1, 1, 1, 1) > 0
    assert lib.d3d_heatmap_peaks_workspace_bytes(1, 2, 2 ** 15, 2 ** 15, 1) == 0          # C * H * W = 2^31
    assert lib.d3d_heatmap_peaks_workspace_bytes(1, 1, 8, 8, 4097) == 0


def test_operators_are_exported():
    import d3d_amd.box as box
    for name in ("heatmap_peaks", "gather_at_peaks", "circle_nms", "gaussian_heatmap", "gaussian_radius", "HeatmapPeaks",
                 "heatmap_peaks_max", "circle_nms_max"):
        assert name in box.__all__ and getattr(box, name) is not None
    assert "sigmoid" in box.heatmap_peaks.__doc__ and "SQUARED" in box.circle_nms.__doc__
    assert box.heatmap_peaks_max() == 4096 and box.circle_nms_max() == 4096


# ---------------------------------------------------------------- the models against independent formulations
@pytest.mark.parametrize("shape", cases.PEAK_SHAPES[:4] + ((1, 2, 40, 48),), ids=str)
def test_peak_model_is_max_pool_equality_and_topk(shape):
    b, c, h, w = shape
    for name, heat in cases.peak_scenes(shape).items():
        t = torch.from_numpy(heat)
        for kernel in cases.KERNELS:
            mask = ref.peak_mask(heat, kernel)
            pooled = torch.max_pool2d(t, kernel, 1, kernel // 2)
            assert np.array_equal(mask, (pooled == t).numpy()), (name, kernel)              # NaN, +-inf, -0.0 included
            k = min(50, c * h * w)
            flat, counts = ref.heatmap_peaks_model(heat, k, kernel)
            assert np.array_equal(counts, np.minimum(mask.reshape(b, -1).sum(1), k))
            vals = np.take_along_axis(heat.reshape(b, -1), np.where(flat < 0, 0, flat), 1)
            for s in range(b):
                got = vals[s, :counts[s]]
                assert np.all(ref.desc_key(got)[:-1] <= ref.desc_key(got)[1:])                # descending, -0 == +0
                assert np.all(flat[s, counts[s]:] == -1) and len(set(flat[s, :counts[s]])) == counts[s]
                same = ref.desc_key(got)[:-1] == ref.desc_key(got)[1:]
                assert np.all(flat[s, :counts[s]][:-1][same] < flat[s, :counts[s]][1:][same])  # ties: ascending flat index
                assert mask.reshape(b, -1)[s, flat[s, :counts[s]]].all()
            if name not in cases.TIE_FREE:
                continue
            # no ties: torch.topk of the masked map gives the same values and the same cells ...
            masked = torch.where(torch.from_numpy(mask), t, torch.full_like(t, -np.inf)).reshape(b, -1)
            tv, ti = torch.topk(masked, k, dim=1)
            for s in range(b):
                m = counts[s]
                assert np.array_equal(tv[s, :m].numpy(), vals[s, :m]) and np.array_equal(ti[s, :m].numpy(), flat[s, :m])
            # ... and so does OpenPCDet's two-stage top-k (per class, then over the classes' winners)
            k1 = min(k, h * w)
            cv, ci = torch.topk(masked.reshape(b, c, -1), k1, dim=2)
            sv, si = torch.topk(cv.reshape(b, -1), k, dim=1)
            cls = si // k1
            cell = ci.reshape(b, -1).gather(1, si)
            classes, ys, xs = ref.unravel_peaks(flat, shape)
            for s in range(b):
                m = counts[s]
                assert np.array_equal(sv[s, :m].numpy(), vals[s, :m]) and np.array_equal(cls[s, :m].numpy(), classes[s, :m])
                assert np.array_equal((cell[s, :m] // w).numpy(), ys[s, :m]) and np.array_equal((cell[s, :m] % w).numpy(), xs[s, :m])


def test_peak_model_threshold_and_prefix():
    heat = cases.peak_scenes((2, 3, 37, 53))["random"]
    flat, counts = ref.heatmap_peaks_model(heat, 4096, 3)
    for k in (1, 7, 64):
        f, c = ref.heatmap_peaks_model(heat, k, 3)
        assert np.array_equal(f, flat[:, :k]) and np.array_equal(c, np.minimum(counts, k))     # a smaller k is a prefix
    best = heat.reshape(2, -1)[0, flat[0, :8]]
    f, c = ref.heatmap_peaks_model(heat[:1], 10, 3, threshold=float(best[5]))
    assert c[0] == 5 and np.array_equal(f[0, :5], flat[0, :5]) and np.all(f[0, 5:] == -1)       # `>`: the value itself is out
    assert ref.heatmap_peaks_model(heat[:1], 10, 3, threshold=float(best[0]))[1][0] == 0
    const = np.full((1, 2, 5, 6), 0.5, np.float32)
    f, c = ref.heatmap_peaks_model(const, 7, 3)
    assert f[0].tolist() == list(range(7)) and c[0] == 7                                         # all ties: the index decides
    assert ref.heatmap_peaks_model(np.full((1, 1, 2, 2), -np.inf, np.float32), 3, 3)[1][0] == 3  # -inf is a value ...
    assert ref.heatmap_peaks_model(np.full((1, 1, 2, 2), -np.inf, np.float32), 3, 3, -np.inf)[1][0] == 0


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
def test_circle_models_agree(dtype):
    for n in (0, 1, 63, 64, 65, 128, 400):
        for levels in (None, 16):
            rows, scores = cases.circle_lattice(n, dtype, levels=levels or 0, side=None)
            for t, cap in ((4.0, None), (1.0, 1), (9.0, 83), (0.0, None)):
                a = ref.circle_nms_model(rows, scores, t, max_keep=cap)
                assert np.array_equal(a, ref.circle_nms_matrix(rows, scores, t, max_keep=cap)), (n, levels, t, cap)
                if n:
                    assert a[ref.argsort_desc_model(scores)[0]] and (cap is None or a.sum() <= cap)
    rows, scores = cases.circle_lattice(300, dtype, levels=8)
    rows[::7, 0] = np.nan
    scores[::11] = np.nan
    offsets = [0, 0, 5, 5, 70, 200, 300, 300]
    a = ref.circle_nms_model(rows, scores, 4.0, offsets, 20)
    assert np.array_equal(a, ref.circle_nms_matrix(rows, scores, 4.0, offsets, 20))
    for lo, hi in zip(offsets, offsets[1:]):                     # never across segments: a segment alone gives the same rows
        assert np.array_equal(a[lo:hi], ref.circle_nms_model(rows[lo:hi], scores[lo:hi], 4.0, max_keep=20))
    for first in (10, 62, 63):
        centers, scores, t, keep = cases.circle_chain(dtype, first)
        assert np.array_equal(ref.circle_nms_model(centers, scores, t), keep)
    # a row exactly at the threshold is suppressed (<=); duplicates: the first visited stays
    pts = np.array([[0, 0], [2, 0], [0, 0], [5, 5]], dtype)
    assert ref.circle_nms_model(pts, np.array([4, 3, 2, 1], dtype), 4.0).tolist() == [True, False, False, True]
    assert ref.circle_nms_model(pts, np.array([1, 1, 1, 1], dtype), 0.0).tolist() == [True, True, False, True]


def _centernet_draw(heatmap, center, radius):
    """CenterNet's gaussian2D + draw_umich_gaussian (k = 1), float64 as numpy computes it; the caller passes only boxes whose window
    meets the map (the slices of the original wrap around for the others)"""
    diameter = 2 * radius + 1
    sigma = diameter / 6
    y, x = np.ogrid[-radius:radius + 1, -radius:radius + 1]
    gaussian = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    gaussian[gaussian < np.finfo(gaussian.dtype).eps * gaussian.max()] = 0
    x, y = center
    height, width = heatmap.shape
    left, right = min(x, radius), min(width - x, radius + 1)
    top, bottom = min(y, radius), min(height - y, radius + 1)
    masked_heatmap = heatmap[y - top:y + bottom, x - left:x + right]
    masked_gaussian = gaussian[radius - top:radius + bottom, radius - left:radius + right]
    assert masked_heatmap.shape == masked_gaussian.shape and min(masked_gaussian.shape) > 0
    np.maximum(masked_heatmap, masked_gaussian, out=masked_heatmap)


def test_drawing_model_is_centernets_gaussian():
    b, c, h, w = cases.DRAW_SHAPE
    for name, (centers, radii, classes, offsets) in cases.draw_scenes().items():
        got = ref.gaussian_heatmap_model(centers, radii, classes, cases.DRAW_SHAPE, offsets)
        want = np.zeros(cases.DRAW_SHAPE, np.float64)
        drawn = np.zeros(cases.DRAW_SHAPE, bool)
        for s in range(b):
            for i in range(offsets[s], offsets[s + 1]):
                cx, cy, r = int(centers[i, 0]), int(centers[i, 1]), int(radii[i])
                if r > 200 or abs(cx) > 10 ** 6 or abs(cy) > 10 ** 6:            # (the float formulation builds a (2 r + 1)^2 patch)
                    x0, x1, y0, y1 = max(cx - r, 0), min(cx + r, w - 1), max(cy - r, 0), min(cy + r, h - 1)
                    if x0 <= x1 and y0 <= y1:
                        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
                        view = want[s, classes[i], y0:y1 + 1, x0:x1 + 1]
                        np.maximum(view, np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * ((2 * r + 1) / 6) ** 2)), out=view)
                elif cx + r >= 0 and cx - r <= w - 1 and cy + r >= 0 and cy - r <= h - 1:
                    _centernet_draw(want[s, classes[i]], (cx, cy), r)
                if 0 <= cx < w and 0 <= cy < h:
                    drawn[s, classes[i], cy, cx] = True
        assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-6, atol=0), name       # within the float formula's rounding
        assert np.array_equal(got == 0, want == 0) and np.all(got[drawn] == 1.0), name          # the eps mask never fires; centres
    assert ref.gaussian_heatmap_model(*cases.draw_scenes()["no_boxes"][:3], cases.DRAW_SHAPE, [0, 0, 0, 0]).max() == 0


def test_gaussian_radius_is_centernets_formula():
    from d3d_amd.box import gaussian_radius

    def centernet(height, width, min_overlap):
        a1, b1, c1 = 1, height + width, width * height * (1 - min_overlap) / (1 + min_overlap)
        r1 = (b1 + np.sqrt(b1 ** 2 - 4 * a1 * c1)) / 2
        a2, b2, c2 = 4, 2 * (height + width), (1 - min_overlap) * width * height
        r2 = (b2 + np.sqrt(b2 ** 2 - 4 * a2 * c2)) / 2
        a3, b3, c3 = 4 * min_overlap, -2 * min_overlap * (height + width), (min_overlap - 1) * width * height
        r3 = (b3 + np.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
        return min(r1, r2, r3)

    w = np.array([1.0, 4.6, 19.5, 40.0, 3.0, 200.0])
    l = np.array([1.0, 2.1, 8.25, 12.0, 90.0, 180.0])
    for mo in (0.1, 0.5, 0.7):
        got = gaussian_radius(torch.from_numpy(w), torch.from_numpy(l), mo, min_radius=2)
        assert got.dtype == torch.int32
        assert got.tolist() == [max(int(centernet(a, b, mo)), 2) for a, b in zip(l, w)]
    assert gaussian_radius(w.astype(np.float32), l.astype(np.float32)).shape == (6,)
    assert int(gaussian_radius(0.5, 0.5, min_radius=3)) == 3


def test_gather_at_peaks_is_plain_indexing():
    from d3d_amd.box import HeatmapPeaks, gather_at_peaks
    maps = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5).requires_grad_()
    ys = torch.tensor([[0, 3, -1], [2, -1, 1]], dtype=torch.int32)
    xs = torch.tensor([[4, 0, -1], [2, -1, 1]], dtype=torch.int32)
    peaks = HeatmapPeaks(None, None, ys, xs, None)
    out = gather_at_peaks(maps, peaks)
    assert out.shape == (2, 3, 3)
    for s in range(2):
        for j in range(3):
            want = maps[s, :, ys[s, j], xs[s, j]] if ys[s, j] >= 0 else torch.zeros(3)
            assert torch.equal(out[s, j], want)
    out.sum().backward()
    assert maps.grad.sum() == 4 * 3                                                     # four present slots, three channels each
    assert isinstance(gather_at_peaks(maps.detach().numpy(), peaks), np.ndarray)


# ---------------------------------------------------------------- refusals, before a GPU is needed
@pytest.fixture
def no_device(monkeypatch):
    """the library and the device are out of reach: validation that touches either fails the test"""
    from d3d_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("validation reached the library / the device")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "require_gpu", refuse)


def test_heatmap_peaks_refusals(no_device):
    from d3d_amd.box import heatmap_peaks
    heat = torch.zeros(1, 2, 8, 8)
    for k in (0, 4097, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="k must be"):
            heatmap_peaks(heat, k)
    for kernel in (0, 2, 4, 9, -3, 3.0):
        with pytest.raises(ValueError, match="kernel must be"):
            heatmap_peaks(heat, 5, kernel)
    for bad in (heat.double(), heat.long(), np.zeros((1, 2, 8, 8), np.float64), np.zeros((1, 2, 8, 8), np.int32)):
        with pytest.raises(ValueError, match="heat must be float32"):
            heatmap_peaks(bad, 5)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        heatmap_peaks(torch.zeros(2, 8, 8), 5)
    with pytest.raises(ValueError, match="empty plane"):
        heatmap_peaks(torch.zeros(1, 2, 0, 8), 5)
    with pytest.raises(ValueError, match="2\\^31 - 1"):                                  # by shape only: no such map is allocated
        heatmap_peaks(torch.zeros(1).expand(1, 2, 2 ** 15, 2 ** 15), 5)
    with pytest.raises(ValueError, match="NaN"):
        heatmap_peaks(heat, 5, threshold=float("nan"))
    with pytest.raises(TypeError):
        heatmap_peaks([[[[0.0]]]], 1)
    with pytest.raises(AssertionError, match="validation reached"):                      # valid arguments: only now the library
        heatmap_peaks(heat, 4096, 7, 0.1)


def test_circle_nms_refusals(no_device):
    from d3d_amd.box import circle_nms
    c, s = torch.zeros(6, 2), torch.zeros(6)
    with pytest.raises(ValueError, match="not both"):
        circle_nms(c, s, 1.0, offsets=[0, 6], groups=torch.zeros(6, dtype=torch.int64))
    for bad_c, bad_s in ((c.half(), s.half()), (c.long(), s.long()), (c, s.double()), (c.double(), s)):
        with pytest.raises(ValueError, match="float32|same dtype"):
            circle_nms(bad_c, bad_s, 1.0)
    with pytest.raises(ValueError, match="D >= 2"):
        circle_nms(torch.zeros(6, 1), s, 1.0)
    with pytest.raises(ValueError, match="inconsistent"):
        circle_nms(c, s[:5], 1.0)
    with pytest.raises(ValueError, match="inconsistent"):
        circle_nms(c, s, 1.0, groups=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(TypeError):
        circle_nms(c, s, 1.0, groups=torch.zeros(6))
    for offsets in ([0, 5], [1, 6], [0, 4, 3, 6], [0, 7], [[0, 6]]):                      # offsets that do not cover the rows
        with pytest.raises(ValueError, match="offsets"):
            circle_nms(c, s, 1.0, offsets=offsets)
    for cap in (-1, 1.5, True):
        with pytest.raises(ValueError, match="max_keep"):
            circle_nms(c, s, 1.0, max_keep=cap)
    big_c, big_s = torch.zeros(4097 + 10, 2), torch.zeros(4097 + 10)
    with pytest.raises(ValueError, match="4097 rows"):
        circle_nms(big_c, big_s, 1.0, offsets=[0, 10, 4107])
    with pytest.raises(ValueError, match="4097 rows"):
        circle_nms(big_c, big_s, 1.0, groups=torch.cat([torch.full((10,), -3), torch.full((4097,), 9)]))
    with pytest.raises(ValueError, match="4107 rows"):
        circle_nms(big_c.numpy(), big_s.numpy(), 1.0)
    # nothing to do: decided on the host, answered where the centers live
    assert circle_nms(torch.zeros(0, 2), torch.zeros(0), 1.0).shape == (0,)
    got = circle_nms(np.zeros((0, 3)), np.zeros(0), 1.0, groups=np.zeros(0, np.int8))
    assert isinstance(got, np.ndarray) and got.dtype == bool and got.shape == (0,)
    with pytest.raises(AssertionError, match="validation reached"):
        circle_nms(c, s, 1.0, offsets=[0, 2, 2, 6], max_keep=3)


def test_gaussian_heatmap_refusals(no_device):
    from d3d_amd.box import gaussian_heatmap
    xy, r, cl = torch.zeros(4, 2, dtype=torch.int64), torch.ones(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    shape = (1, 3, 16, 16)
    for bad in (torch.tensor([0, 0, 3, 0]), torch.tensor([0, -1, 0, 0])):                 # a class outside [0, C)
        with pytest.raises(ValueError, match="classes holds"):
            gaussian_heatmap(xy, r, bad, shape)
    for bad in (torch.tensor([1, 4096, 1, 1]), torch.tensor([1, 1, -1, 1])):              # a radius of 4096
        with pytest.raises(ValueError, match="radii holds"):
            gaussian_heatmap(xy, bad, cl, shape)
    for args in ((xy.float(), r, cl), (xy, r.float(), cl), (xy, r, cl.bool()), (xy.numpy().astype(np.float64), r.numpy(), cl.numpy())):
        with pytest.raises(ValueError, match="integers"):
            gaussian_heatmap(*args, shape)
    with pytest.raises(ValueError, match=r"\[M, 2\]"):
        gaussian_heatmap(torch.zeros(4, 3, dtype=torch.int64), r, cl, shape)
    with pytest.raises(ValueError, match="one row per box"):
        gaussian_heatmap(xy, r[:3], cl, shape)
    for bad_shape in ((3, 16, 16), (1, 3, 16, -1), (1, 3, 16, 1.0), (70000, 1, 4, 4), (1, 1, 2 ** 30 + 1, 1)):
        with pytest.raises(ValueError, match="shape must be|takes B, C"):
            gaussian_heatmap(xy, r, cl, bad_shape)
    with pytest.raises(ValueError, match="needs offsets"):
        gaussian_heatmap(xy, r, cl, (2, 3, 16, 16))
    for offsets in ([0, 3], [0, 2, 5], [1, 4], [0, 3, 2, 4]):                              # offsets that do not cover the boxes
        with pytest.raises(ValueError, match="offsets"):
            gaussian_heatmap(xy, r, cl, (len(offsets) - 1, 3, 16, 16), offsets)
    with pytest.raises(ValueError, match="names 2 samples"):
        gaussian_heatmap(xy, r, cl, (3, 3, 16, 16), [0, 2, 4])
    with pytest.raises(AssertionError, match="validation reached"):
        gaussian_heatmap(xy, r, cl, (2, 3, 16, 16), [0, 1, 4])


# ---------------------------------------------------------------- the C entries' argument codes (they run before the first HIP call)
_BAD, _UNSUP, _WS = -1, -2, -3


def test_c_entries_reject_bad_arguments_before_any_launch():
    """one wrong argument per call, a host arena standing in for every device pointer; not for a machine with a GPU, where a table of
    deliberately wrong arguments has no business"""
    if torch.cuda.is_available():
        pytest.skip("host-side argument checks: run where there is no GPU")
    from d3d_amd import _lib
    lib = _lib.load()
    arena = (ctypes.c_char * (1 << 20))()
    dev = ctypes.addressof(arena)
    need = lib.d3d_heatmap_peaks_workspace_bytes(2, 3, 16, 16, 8)
    assert 0 < need <= len(arena)

    def peaks(**wrong):
        a = dict(heat=dev, b=2, c=3, h=16, w=16, dtype=_lib.F32, k=8, kernel=3, has=0, thr=0.0, scores=dev, classes=dev, ys=dev, xs=dev,
                 counts=dev, ws=dev, ws_bytes=need, stream=None)
        a.update(wrong)
        return lib.d3d_heatmap_peaks(*a.values())

    for wrong, code in ((dict(b=-1), _BAD), (dict(c=0), _BAD), (dict(h=0), _BAD), (dict(w=-2), _BAD), (dict(k=0), _BAD), (dict(kernel=2), _BAD),
                        (dict(kernel=9), _BAD), (dict(has=2), _BAD), (dict(heat=None), _BAD), (dict(scores=None), _BAD),
                        (dict(counts=None), _BAD), (dict(xs=None), _BAD), (dict(dtype=_lib.F64), _UNSUP), (dict(dtype=_lib.F32_WIDE), _UNSUP),
                        (dict(k=4097), _UNSUP), (dict(b=65536), _UNSUP), (dict(c=2, h=2 ** 15, w=2 ** 15), _UNSUP),
                        (dict(ws=None), _WS), (dict(ws_bytes=need - 1), _WS), (dict(k=0, ws=None), _BAD), (dict(dtype=9, ws_bytes=0), _UNSUP)):
        assert peaks(**wrong) == code, wrong
    assert peaks(b=0, heat=None, scores=None, ws=None) == _lib.OK

    def circle(**wrong):
        a = dict(centers=dev, stride=2, scores=dev, perm=None, seg=dev, n=10, segments=2, max_segment=8, dtype=_lib.F32, thr=1.0, max_keep=5,
                 keep=dev, stream=None)
        a.update(wrong)
        return lib.d3d_circle_nms(*a.values())

    for wrong, code in ((dict(n=-1), _BAD), (dict(segments=-1), _BAD), (dict(stride=1), _BAD), (dict(max_segment=-1), _BAD),
                        (dict(max_keep=-1), _BAD), (dict(centers=None), _BAD), (dict(scores=None), _BAD), (dict(seg=None), _BAD),
                        (dict(keep=None), _BAD), (dict(dtype=_lib.F16), _UNSUP), (dict(dtype=_lib.F64_M32), _UNSUP),
                        (dict(max_segment=4097), _UNSUP), (dict(n=2 ** 31), _UNSUP), (dict(segments=2 ** 31), _UNSUP),
                        (dict(stride=1, dtype=_lib.F16), _BAD)):
        assert circle(**wrong) == code, wrong
    for nothing in (dict(n=0), dict(segments=0), dict(max_segment=0)):
        assert circle(centers=None, keep=None, **nothing) == _lib.OK

    def draw(**wrong):
        a = dict(centers=dev, radii=dev, classes=dev, offsets=dev, m=5, b=2, c=3, h=16, w=16, out=dev, stream=None)
        a.update(wrong)
        return lib.d3d_gaussian_heatmap(*a.values())

    for wrong, code in ((dict(m=-1), _BAD), (dict(b=-1), _BAD), (dict(w=-1), _BAD), (dict(offsets=None), _BAD), (dict(out=None), _BAD),
                        (dict(centers=None), _BAD), (dict(radii=None), _BAD), (dict(classes=None), _BAD), (dict(b=65536), _UNSUP),
                        (dict(c=65536), _UNSUP), (dict(h=2 ** 30 + 1), _UNSUP), (dict(m=2 ** 31), _UNSUP)):
        assert draw(**wrong) == code, wrong
    for nothing in (dict(b=0), dict(c=0), dict(h=0), dict(w=0)):
        assert draw(out=None, **nothing) == _lib.OK
