"""GPU: heatmap_peaks, circle_nms and gaussian_heatmap (csrc/center.hip) against the numpy models of center_reference.py on the scenes
of center_cases.py -- bit for bit, except the drawn values: those lie within 1 fp32 ulp of the model (zeros and the 1.0 at centres
exact), because model and kernel evaluate the same fp64 expression with two exp's that are each within 1 fp64 ulp."""
import numpy as np
import pytest
import torch

import center_cases as cases
import center_reference as ref
from d3d_amd import _lib
from d3d_amd.box import circle_nms, gather_at_peaks, gaussian_heatmap, heatmap_peaks

pytestmark = pytest.mark.gpu
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(t):
    """the bits of a float tensor as an integer numpy array"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


_SCENES, _MODELS = {}, {}


def scene(shape, name, dtype="f32"):
    """one scene as a host tensor of `dtype` (rounded once from the float32 scene), shared"""
    key = (shape, name, dtype)
    if key not in _SCENES:
        if (shape, None) not in _SCENES:
            _SCENES[(shape, None)] = cases.peak_scenes(shape)
        _SCENES[key] = torch.from_numpy(_SCENES[(shape, None)][name]).to(TORCH[dtype])
    return _SCENES[key]


def model(shape, name, dtype, kernel, threshold=None):
    """the model's ranking of a scene for k = 4096, computed once: a smaller k is its prefix (test_center.py checks that)"""
    key = (shape, name, dtype, kernel, threshold)
    if key not in _MODELS:
        _MODELS[key] = ref.heatmap_peaks_model(scene(shape, name, dtype).float().numpy(), 4096, kernel, threshold)
    return _MODELS[key]


def check_peaks(got, heat, flat, counts, k):
    """got == the model's first k ranks; the scores are the input's own bits, the tail is -inf / -1"""
    b = heat.shape[0]
    flat, counts = flat[:, :k], np.minimum(counts, k)
    classes, ys, xs = ref.unravel_peaks(flat, heat.shape)
    assert np.array_equal(got.counts.cpu().numpy(), counts)
    assert np.array_equal(got.classes.cpu().numpy(), classes) and np.array_equal(got.ys.cpu().numpy(), ys)
    assert np.array_equal(got.xs.cpu().numpy(), xs)
    assert got.scores.dtype == heat.dtype and got.classes.dtype == torch.int32 and got.counts.dtype == torch.int32
    want = np.take_along_axis(raw(heat).reshape(b, -1), np.where(flat < 0, 0, flat), 1)
    want[flat < 0] = raw(torch.tensor([-np.inf], dtype=heat.dtype))[0]
    assert np.array_equal(raw(got.scores), want)


@pytest.mark.parametrize("kernel", cases.KERNELS)
@pytest.mark.parametrize("shape", cases.PEAK_SHAPES, ids=str)
def test_peaks_every_scene_and_k(shape, kernel):
    for name in cases.peak_scenes(shape):
        heat = scene(shape, name)
        flat, counts = model(shape, name, "f32", kernel)
        dev = heat.cuda()
        for k in cases.PEAK_KS:                                                # k above the candidates: the -inf / -1 tail, counts
            check_peaks(heatmap_peaks(dev, k, kernel), heat, flat, counts, k)


@pytest.mark.parametrize("dtype", ("f16", "bf16"))
@pytest.mark.parametrize("shape", (cases.PEAK_SHAPES[3], cases.PEAK_SHAPES[4]), ids=str)
def test_peaks_half_types(shape, dtype):
    """the half types are widened exactly: rounding the scene to them makes ties, which the index decides; the bits come back"""
    for name in ("random", "special", "signed_zeros", "top24_shared"):
        heat = scene(shape, name, dtype)
        for kernel in (1, 3):
            flat, counts = model(shape, name, dtype, kernel)
            for k in (7, 500):
                check_peaks(heatmap_peaks(heat.cuda(), k, kernel), heat, flat, counts, k)


@pytest.mark.parametrize("shape", (cases.PEAK_SHAPES[3], cases.PEAK_SHAPES[4]), ids=str)
def test_peaks_thresholds(shape):
    """thresholds that leave 0, 1 and k - 1 candidates in sample 0 (`>`: the threshold's own value is out), and one in the middle"""
    heat = scene(shape, "random")
    flat, counts = model(shape, "random", "f32", 3)
    best = heat.reshape(shape[0], -1)[0, flat[0, :64]].tolist()
    k = 64
    for leaves, thr in ((0, best[0]), (1, best[1]), (k - 1, best[k - 1]), (None, 0.0), (None, float("-inf")), (None, float("inf"))):
        f, c = model(shape, "random", "f32", 3, thr)
        assert leaves is None or c[0] == leaves
        check_peaks(heatmap_peaks(heat.cuda(), k, 3, threshold=thr), heat, f, c, k)
    plate = scene(shape, "plateaus")
    f, c = model(shape, "plateaus", "f32", 5, 0.5)
    check_peaks(heatmap_peaks(plate.cuda(), 500, 5, threshold=0.5), plate, f, c, 500)
    # the threshold is rounded to float32: 0.1 is float32(0.1) = 0.100000001..., which a cell holding float32(0.1) does not exceed
    tenth = torch.full((1, 1, 3, 3), 0.1)
    assert int(heatmap_peaks(tenth.cuda(), 4, 1, threshold=0.1).counts[0]) == 0


def tile_edge_scene(shape, last_in, k):
    """One sample: a background of -1, `above` lone peaks with distinct values above 2 and ties of 1.0 on lone cells on both sides of
    every multiple of 256 flat cells (a wavefront's share of a workgroup's tile of 1024) and on the last cells of the map.  The
    k-th rank falls among the ties: `last_in` -- there are exactly as many ties as ranks left, the map's last cell takes the last
    one; else one tie more, and the last cell is the one left out.  Which cells are lone peaks is for the model to say."""
    c, h, w = shape
    n = c * h * w
    taken = []

    def lone(e):
        p, y, x = e // (h * w), e % (h * w) // w, e % w
        return all(q // (h * w) != p or abs(q % (h * w) // w - y) > 1 or abs(q % w - x) > 1 for q in taken)

    wanted = [n - 1, n - 3, n - 5] + [b + d for b in (256, 512, 768, 1024) for d in (-5, -3, -1, 1, 3)] + list(range(2, 40, 2))
    for e in wanted:
        if 0 <= e < n and e not in taken and lone(e):
            taken.append(e)
    ties = sorted(taken)
    above = k - len(ties) + (0 if last_in else 1)
    heat = np.full(n, -1.0, np.float32)
    heat[ties] = 1.0
    for e in np.random.default_rng(n).permutation(n):
        if len(taken) == len(ties) + above:
            break
        if lone(int(e)):
            taken.append(int(e))
            heat[e] = 2.0 + (len(taken) - len(ties)) / 64.0            # (exact in fp16 and bf16 steps of 1 / 64 below 4)
    assert len(taken) == len(ties) + above and above > 0
    return heat.reshape(shape), ties


@pytest.mark.parametrize("dtype", ("f32", "f16"))
@pytest.mark.parametrize("shape", ((1, 1, 1, 1023), (2, 1, 32, 32), (1, 1, 25, 41)), ids=str)
def test_peaks_ties_across_the_tile_edge(shape, dtype):
    """c h w of 1023, 1024 and 1025 cells: the map ends one short of a tile of 1024, on it and one cell into the next.  Which ties of
    the k-th value win is a matter of the lowest flat index, i.e. of the prefix over the rows, wavefronts and tiles before a cell."""
    k, n = 65, int(np.prod(shape[1:]))
    for first_in in (True, False):
        built = [tile_edge_scene(shape[1:], first_in == (b % 2 == 0), k) for b in range(shape[0])]
        heat = torch.from_numpy(np.stack([m for m, _ in built])).to(TORCH[dtype])
        flat, counts = ref.heatmap_peaks_model(heat.float().numpy(), k, 3)
        for b, (_, ties) in enumerate(built):                                  # the scene is what it is meant to be
            last_in = first_in == (b % 2 == 0)
            won = set(flat[b].tolist())
            assert counts[b] == k and ties[-1] == n - 1 and (n - 1 in won) == last_in and set(ties[:-1]) <= won
            assert any(e < 256 for e in ties) and any(768 <= e < 1024 for e in ties) and (n <= 1024 or ties[-1] == 1024)
        check_peaks(heatmap_peaks(heat.cuda(), k, 3), heat, flat, counts, k)


def test_peaks_inputs_and_determinism():
    shape = cases.PEAK_SHAPES[3]
    heat = scene(shape, "plateaus")
    flat, counts = model(shape, "plateaus", "f32", 3)
    dev = heat.cuda()
    first = heatmap_peaks(dev, 500, 3)
    again = heatmap_peaks(dev, 500, 3)
    for a, b in zip(first, again):                                             # two runs, equal bits
        assert torch.equal(a, b) and a.is_cuda
    assert torch.equal(dev, heat.cuda())                                       # the map is only read
    # a non-contiguous view: the front makes it contiguous
    wide = torch.zeros(shape[:3] + (2 * shape[3],))
    wide[..., ::2] = heat
    view = wide.cuda()[..., ::2]
    assert not view.is_contiguous()
    check_peaks(heatmap_peaks(view, 65, 3), heat, flat, counts, 65)
    # a host tensor and a numpy array answer on their side
    got = heatmap_peaks(heat, 65, 3)
    assert all(not t.is_cuda for t in got)
    check_peaks(got, heat, flat, counts, 65)
    got = heatmap_peaks(heat.numpy(), 65, 3)
    assert all(isinstance(a, np.ndarray) for a in got)
    check_peaks(type(got)(*[torch.from_numpy(a) for a in got]), heat, flat, counts, 65)
    assert heatmap_peaks(torch.zeros((0, 2, 4, 4)).cuda(), 3).scores.shape == (0, 3)
    # gather_at_peaks reads the regression maps at the peaks; missing slots give zero rows
    maps = torch.arange(float(np.prod(shape))).reshape(shape).cuda()
    peaks = heatmap_peaks(scene(shape, "borders").cuda(), 64, 3, threshold=0.0)       # (the background is one plateau of peaks)
    rows = gather_at_peaks(maps, peaks)
    n0 = int(peaks.counts[0])
    assert 0 < n0 < 64 and rows.shape == (shape[0], 64, shape[1]) and torch.all(rows[0, n0:] == 0)
    assert torch.equal(rows[0, :n0, 1], maps[0, 1].reshape(-1)[(peaks.ys[0, :n0] * shape[3] + peaks.xs[0, :n0]).long()])


def test_peaks_raw_entry_keeps_to_its_workspace():
    """the C entry on its own buffers: the workspace of the size the query names, a guard band behind it that must stay untouched"""
    lib = _lib.load()
    shape, k, guard = cases.PEAK_SHAPES[4], 4096, 4096
    heat = scene(shape, "three_values")
    flat, counts = model(shape, "three_values", "f32", 7)
    b, c, h, w = shape
    need = lib.d3d_heatmap_peaks_workspace_bytes(b, c, h, w, k)
    assert 0 < need < b * (3 * 4096 * 4 + (c * h * w // 1024 + 1) * 8 + k * 8 + 8 * 256)        # bins + tiles + k, not the map
    dev = heat.cuda()
    ws = torch.full((need + guard,), 0xa5, dtype=torch.uint8, device="cuda")
    scores = torch.empty((b, k), device="cuda")
    classes, ys, xs = (torch.empty((b, k), dtype=torch.int32, device="cuda") for _ in range(3))
    cnt = torch.empty((b,), dtype=torch.int32, device="cuda")
    args = [_lib.ptr(dev), b, c, h, w, _lib.F32, k, 7, 0, 0.0, _lib.ptr(scores), _lib.ptr(classes), _lib.ptr(ys), _lib.ptr(xs), _lib.ptr(cnt),
            _lib.ptr(ws)]
    assert lib.d3d_heatmap_peaks(*args, need - 1, _lib.stream_ptr()) == _lib.ERR_WORKSPACE
    assert lib.d3d_heatmap_peaks(*args, need, _lib.stream_ptr()) == _lib.OK
    from d3d_amd.box import HeatmapPeaks
    check_peaks(HeatmapPeaks(scores, classes, ys, xs, cnt), heat, flat, counts, k)
    assert bool((ws[need:] == 0xa5).all())


# ---------------------------------------------------------------- circle NMS
NP = {"f32": np.float32, "f64": np.float64}


@pytest.mark.parametrize("dtype", ("f32", "f64"))
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 128, 1000, 4096))
def test_circle_nms_lattices(n, dtype):
    """integer lattices: every d2 is exact, duplicate centres and rows exactly at the threshold are common; distinct and tied scores;
    [N, 4] rows as they lie"""
    for levels in (None, 16):
        rows, scores = cases.circle_lattice(n, NP[dtype], levels=levels)
        d_rows, d_scores = cuda(rows), cuda(scores)
        for t, cap in ((4.0, None), (9.0, 83), (1.0, 1), (0.0, 10 ** 6)):
            want = ref.circle_nms_model(rows, scores, t, max_keep=cap)
            got = circle_nms(d_rows, d_scores, t, max_keep=cap)
            assert got.dtype == torch.bool and (got.is_cuda or n == 0) and np.array_equal(got.cpu().numpy(), want), (levels, t, cap)
        if n:                                                                  # max_keep above the survivors changes nothing
            assert int(want.sum()) < 10 ** 6 and np.array_equal(want, ref.circle_nms_model(rows, scores, 0.0))


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_circle_nms_chain_nan_and_fractions(dtype):
    for first in (10, 62, 63, 64):                                             # A suppresses B, B alone would suppress C: C stays
        centers, scores, t, keep = cases.circle_chain(NP[dtype], first)
        assert np.array_equal(circle_nms(cuda(centers), cuda(scores), t).cpu().numpy(), keep), first
    rows, scores = cases.circle_lattice(700, NP[dtype], levels=8)
    rows[::7, 0] = np.nan                                                      # a NaN d2 suppresses nothing, either way round
    rows[3::31, 1] = np.inf
    scores[::11] = np.nan                                                      # NaN scores are visited first
    want = ref.circle_nms_model(rows, scores, 4.0)
    assert np.array_equal(circle_nms(cuda(rows), cuda(scores), 4.0).cpu().numpy(), want)
    # fractions: d2 is rounded, once per operation in the dtype, and so is the threshold
    rng = np.random.default_rng(7)
    pts = (rng.uniform(0, 30, (900, 2))).astype(NP[dtype])
    sc = rng.uniform(0, 1, 900).astype(NP[dtype])
    for t in (0.1, 1.7, 1e-3):
        want = ref.circle_nms_model(pts, sc, t, max_keep=83)
        assert np.array_equal(circle_nms(cuda(pts), cuda(sc), t, max_keep=83).cpu().numpy(), want)
    got = circle_nms(pts, sc, 1.7)                                             # numpy in, numpy out
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref.circle_nms_model(pts, sc, 1.7))
    wide = cuda(np.concatenate([pts, pts], 1))[:, 1:3]                         # a column slice of wider rows: read as it lies
    assert np.array_equal(circle_nms(wide, cuda(sc), 1.7).cpu().numpy(), ref.circle_nms_model(np.stack([pts[:, 1], pts[:, 0]], 1), sc, 1.7))


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_circle_nms_segments_and_groups(dtype):
    rows, scores = cases.circle_lattice(1500, NP[dtype], levels=32, side=24)
    offsets = [0, 0, 5, 5, 69, 70, 200, 1300, 1300, 1500, 1500]               # ragged, with empty segments
    for cap in (None, 1, 83):
        want = ref.circle_nms_model(rows, scores, 4.0, offsets, cap)
        got = circle_nms(cuda(rows), cuda(scores), 4.0, offsets=offsets, max_keep=cap)
        assert np.array_equal(got.cpu().numpy(), want)
        again = circle_nms(cuda(rows), cuda(scores), 4.0, offsets=torch.tensor(offsets), max_keep=cap)
        assert torch.equal(got, again)                                         # two runs, equal bits
        # the same segments named by group values: negative, with gaps
        ids = np.repeat(np.array([-9, -7, -3, -2, 0, 5, 9, 1000, 1001, 2 ** 40]), np.diff(offsets))
        assert np.array_equal(circle_nms(cuda(rows), cuda(scores), 4.0, groups=cuda(ids), max_keep=cap).cpu().numpy(), want)
    # unsorted groups: every group is its rows in ascending row order
    rng = np.random.default_rng(3)
    ids = rng.choice(np.array([-4, 0, 3, 77], np.int32), 1500)
    got = circle_nms(cuda(rows), cuda(scores), 4.0, groups=cuda(ids), max_keep=40).cpu().numpy()
    for g in np.unique(ids):
        idx = np.flatnonzero(ids == g)
        assert np.array_equal(got[idx], ref.circle_nms_model(rows[idx], scores[idx], 4.0, max_keep=40))
    with pytest.raises(ValueError, match="4097 rows"):
        circle_nms(torch.zeros((4097, 2), device="cuda"), torch.zeros((4097,), device="cuda"), 1.0)


# ---------------------------------------------------------------- drawing
def test_gaussian_heatmap_scenes():
    for name, (centers, radii, classes, offsets) in cases.draw_scenes().items():
        want = ref.gaussian_heatmap_model(centers, radii, classes, cases.DRAW_SHAPE, offsets)
        got = gaussian_heatmap(cuda(centers), cuda(radii), cuda(classes), cases.DRAW_SHAPE, offsets)
        assert got.shape == cases.DRAW_SHAPE and got.dtype == torch.float32 and got.is_cuda
        g = got.cpu().numpy()
        # 1 ulp: the same fp64 expression on both sides, a correctly rounded division, two exp's within 1 fp64 ulp each -> fp64
        # results at most 2 fp64 ulps apart -> equal or adjacent after the rounding to fp32
        assert np.array_equal(g == 0, want == 0), name                         # every zero is written, and nothing else is zero
        assert ref.ulp_distance(g, want).max() <= 1, name
        b = np.searchsorted(offsets, np.arange(len(centers)), side="right") - 1
        for i in range(len(centers)):                                          # the 1.0 at every centre inside the map, exactly
            if 0 <= centers[i, 0] < cases.DRAW_SHAPE[3] and 0 <= centers[i, 1] < cases.DRAW_SHAPE[2]:
                assert g[b[i], classes[i], centers[i, 1], centers[i, 0]] == 1.0
        assert torch.equal(got, gaussian_heatmap(cuda(centers), cuda(radii), cuda(classes), cases.DRAW_SHAPE, offsets))      # determinism
        host = gaussian_heatmap(centers, radii.astype(np.int16), classes.astype(np.uint8), cases.DRAW_SHAPE, offsets)      # numpy, any ints
        assert isinstance(host, np.ndarray) and np.array_equal(host, g)
    one = gaussian_heatmap(torch.tensor([[5, 6]]), torch.tensor([2]), torch.tensor([0]), (1, 1, 9, 11))      # no offsets: one sample
    assert not one.is_cuda and one[0, 0, 6, 5] == 1.0 and int((one > 0).sum()) == 25


def test_centre_head_chain():
    """draw separated boxes -> the peaks are exactly the centres and classes with score 1.0 -> circle NMS merges the two close ones"""
    centers = np.array([[10, 8], [40, 8], [25, 20], [12, 30], [14, 31], [45, 33]], np.int64)
    radii = np.array([2, 3, 2, 1, 1, 2], np.int64)
    classes = np.array([0, 1, 2, 0, 1, 2], np.int64)
    shape = (1, 3, 37, 53)
    target = gaussian_heatmap(cuda(centers), cuda(radii), cuda(classes), shape)
    peaks = heatmap_peaks(target, len(centers), kernel=3, threshold=0.5)
    assert int(peaks.counts[0]) == len(centers) and torch.all(peaks.scores == 1.0)
    order = np.lexsort((centers[:, 0], centers[:, 1], classes))               # all scores tie: ascending flat index (class, y, x)
    assert np.array_equal(peaks.classes[0].cpu().numpy(), classes[order])
    assert np.array_equal(peaks.xs[0].cpu().numpy(), centers[order, 0]) and np.array_equal(peaks.ys[0].cpu().numpy(), centers[order, 1])
    xy = torch.stack([peaks.xs[0], peaks.ys[0]], 1).float()
    keep = circle_nms(xy, peaks.scores[0], 5.0)                                # (12, 30) and (14, 31): d2 = 5
    want = ref.circle_nms_model(xy.cpu().numpy(), peaks.scores[0].cpu().numpy(), 5.0)
    assert np.array_equal(keep.cpu().numpy(), want) and int(keep.sum()) == len(centers) - 1
    assert not bool(keep[int(np.flatnonzero((classes[order] == 1) & (centers[order, 0] == 14))[0])])
