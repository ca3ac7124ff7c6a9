"""d3d_pdist2dr_forward / _backward (boxloss.hip k_pdist<T, K>, k_pdist_grad<T>; geom.hpp point_box_distance_local,
point_box_distance<T, GRAD>) and box2dr_pdist / box3dr_pdist on every launch route, against the fp64 model of
tests/pdist_reference.py (tests/test_pdist_reference.py holds that model against oracle.pdist2dr without a GPU).

What each test reaches that the suite did not:
  test_forward_every_route        k_pdist<T, 1> (n % 4 != 0) and <T, 4>, one row / one column, partial last row tile and last
                                  column block, fp32 iedge, sign and feature against the model, poisoned outputs
  test_routes_agree_bit_for_bit   K = 1 chosen by the alignment of dist / iedge alone, iedge == NULL, guard elements
  test_non_positive_sizes         the per-edge branch of the forward kernel (w <= 0 or h <= 0), both kinds in one row tile
  test_exact_ties                 "the lower index on a tie" inside, edges / corners / extended sides exactly on the boundary
  test_empty_and_refused          n == 0, m == 0, more than 65535 row tiles (forward and backward: nothing written)
  test_backward_every_weight      fp32 backward, the g != 0 skip, the s != 0 guard, padding lanes, the partial row tile, the
                                  entry's clearing of its outputs; forward (closed form) and backward (edge loop) features
  test_autograd_and_shim          PDist2DR.backward and both argument orders of box_impl against the raw entry's outputs
  test_box3dr_forward / _backward all three axes, points above / below / beside, gradients of the composition

Bounds.  Values: fp64 1e-12 * scale, fp32 C * 2^-23 * scale with scale = |px| + |py| + |cx| + |cy| + |w| + |h| and C = 4 x the
worst deviation of the compiled fp32 oracle from the fp64 one on these inputs, recomputed at import (FWD_RATIO: 1.25 on
these seeds, both offsets, so C = 5.0; the factor 4 because the kernel's closed form is another, equally short formula.
The kernels: 1.24 in fp32, 1.36 eps in fp64).  Features and sign: exact on decided pairs (margin 1e-3, see
pdist_reference.features); undecided pairs are at most 1 % of a case (both offsets and types alike: 0/1, 0/3, 1/260,
32/16320, 42/16191, 9/2046, 4/1024, 407/132225, 377/135061, and 205/66560 at 1024 x 65 -- 0.3 % in all).
Gradients: |got - ref| <= C_g * eps * S + tiny.  S comes from the model's per-pair terms (pdist_reference._sums): the sum
of |g_ij| times the length of the pair's derivative, and times the lever for the angle.  (Summed per box parameter instead,
S is 0 where a derivative vanishes by construction -- d / dh beside the right edge -- while a routine in world coordinates
leaves eps * |g| there, and the model's own fp32 ratio reaches 118 for the angle where one pair weighs on a box.)  C_g in
fp32 = 4 x the worst err / (eps * S) of the model itself run in torch float32 on the CPU over the backward cases, one
factor for the points and one per box parameter (_cg32; measured ratios: points 8.96 -- 1.1 on dense weights --, boxes
1.29, 0.90, 0.46, 0.49, 0.82).  C_g in fp64 = the same ratio of the oracle's central differences (h = 1e-6: 3.8e8) or 64
where that is smaller, so 64.  tiny = the smallest normal number.  Pairs within the margin of the medial axis or of the
boundary carry no weight: 0.14 % .. 0.16 % of a case (cap 1 %); for box3dr_pdist, with the composition's conditions,
0.55 % .. 0.65 %.
What these tests found in point_box_distance<T, true> (geom.hpp): beside an edge, within sqrt(eps) of the point's distance
from the edge's end, the corner's squared distance rounds to the edge's and the first minimum kept the corner, whose
gradient is sqrt(eps) = 3e-4 off in fp32 -- 21 .. 59 eps * S on a point's gradient at these shapes, against 0.5 from the
arithmetic and 2 .. 4 from adding in fp32.  A corner is now kept only beyond the ends of both its edges, and an edge is
2u or 2v, not the difference of two corners (a box 0.1 x 5: 50 eps on its normal)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import pdist_reference as ref

pytestmark = pytest.mark.gpu

EPS = {np.float32: 2.0 ** -23, np.float64: 2.0 ** -52}
DTYPES = [np.float32, np.float64]


def _scene(n, m, offset, dtype):
    return ref.scene(n, m, ref.seed_of(n, m), offset, dtype)


def _measure_forward_ratio():
    worst = 0.0
    for offset in ref.OFFSETS:
        for n, m in ref.FORWARD_SHAPES:
            p, b = _scene(n, m, offset, np.float32)
            d32 = oracle.pdist2dr(p, b)[0].astype(np.float64)
            d64 = oracle.pdist2dr(p.astype(np.float64), b.astype(np.float64))[0]
            worst = max(worst, float((np.abs(d32 - d64) / (EPS[np.float32] * ref.scale(p, b))).max()))
    return worst


FWD_RATIO = _measure_forward_ratio()
C_FWD = 4 * FWD_RATIO


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f64(a):
    return np.asarray(a).astype(np.float64)


# ---------------------------------------------------------------- the raw entries on poisoned outputs with guards
_LEAD = 8            # elements in front of an output: 32 bytes and more, so `shift` alone decides the alignment


def _at(buf, first):
    return ctypes.c_void_p(buf.data_ptr() + first * buf.element_size())


def _guards_intact(buf, first, count, poison):
    rest = torch.cat([buf[:first], buf[first + count:]])
    return bool(torch.isnan(rest).all()) if poison != poison else bool((rest == poison).all())


def _raw_forward(pts, boxes, n=None, m=None, shift_dist=0, shift_iedge=0, iedge=True):
    """d3d_pdist2dr_forward on device tensors -> (rc, dist[m,n], iedge[m,n] or None, guards untouched); dist starts
    `shift_dist` elements and iedge `shift_iedge` bytes past an aligned address, inside buffers full of NaN / 0xFF"""
    from d3d_amd import _lib
    lib = _lib.load()
    n = pts.shape[0] if n is None else n
    m = boxes.shape[0] if m is None else m
    dbuf = torch.full((m * n + 3 * _LEAD,), float("nan"), dtype=pts.dtype, device="cuda")
    ebuf = torch.full((m * n + 3 * _LEAD,), 255, dtype=torch.uint8, device="cuda")
    assert dbuf.data_ptr() % 32 == 0 and ebuf.data_ptr() % 4 == 0
    fd, fe = _LEAD + shift_dist, _LEAD + shift_iedge
    rc = lib.d3d_pdist2dr_forward(_at(pts, 0), n, _at(boxes, 0), m, _lib.F64 if pts.dtype == torch.float64 else _lib.F32,
                                  _at(dbuf, fd), _at(ebuf, fe) if iedge else ctypes.c_void_p(0), _lib.stream_ptr())
    torch.cuda.synchronize()
    ok = _guards_intact(dbuf, fd, m * n, float("nan")) and _guards_intact(ebuf, fe, m * n if iedge else 0, 255)
    d = dbuf[fd:fd + m * n].reshape(m, n).cpu().numpy()
    e = ebuf[fe:fe + m * n].reshape(m, n).cpu().numpy()
    return rc, d, (e if iedge else None), ok


def _raw_backward(pts, boxes, g, outs=None):
    """d3d_pdist2dr_backward -> (rc, grad_boxes[m,5], grad_points[n,2], guards untouched, outs); fresh outputs are full of NaN"""
    from d3d_amd import _lib
    lib = _lib.load()
    n, m = pts.shape[0], boxes.shape[0]
    if outs is None:
        outs = tuple(torch.full((k + 3 * _LEAD,), float("nan"), dtype=pts.dtype, device="cuda") for k in (m * 5, n * 2))
    bbuf, pbuf = outs
    rc = lib.d3d_pdist2dr_backward(_at(pts, 0), n, _at(boxes, 0), m, _at(g, 0), _lib.F64 if pts.dtype == torch.float64 else _lib.F32,
                                   _at(bbuf, _LEAD), _at(pbuf, _LEAD), _lib.stream_ptr())
    torch.cuda.synchronize()
    ok = _guards_intact(bbuf, _LEAD, m * 5, float("nan")) and _guards_intact(pbuf, _LEAD, n * 2, float("nan"))
    gb = bbuf[_LEAD:_LEAD + m * 5].reshape(m, 5).cpu().numpy().astype(np.float64)
    gp = pbuf[_LEAD:_LEAD + n * 2].reshape(n, 2).cpu().numpy().astype(np.float64)
    return rc, gb, gp, ok, outs


# ---------------------------------------------------------------- forward
def _value_tol(pts, boxes, dtype):
    return (1e-12 if dtype == np.float64 else C_FWD * EPS[np.float32]) * ref.scale(pts, boxes)


def _check_forward(d, e, pts, boxes, dtype, tag):
    """dist / iedge of regular boxes against the model on the same (rounded) inputs: nothing skipped, values, sign, feature"""
    assert not np.isnan(d).any() and (e is None or (e < 8).all()), tag           # (the poison: NaN / 0xFF)
    p, b = _f64(pts), _f64(boxes)
    model = ref.signed_distance(p, b)
    tol = _value_tol(p, b, dtype)
    err = np.abs(d.astype(np.float64) - model)
    feat, decided, accept = ref.features(p, b)
    print("%s: worst err / tol %.3f (err / (eps scale) %.3f), undecided %d / %d" % (
        tag, float((err / tol).max()), float((err / (EPS[dtype] * ref.scale(p, b))).max()), int((~decided).sum()), decided.size))
    assert (err <= tol).all(), tag
    assert 1 - decided.mean() <= 0.01, tag
    assert np.array_equal((d > 0)[decided], (model > 0)[decided]), tag
    if e is not None:
        bad = ~ref.feature_ok(e, feat, decided, accept)
        assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", ref.OFFSETS)
@pytest.mark.parametrize("shape", ref.FORWARD_SHAPES)
def test_forward_every_route(shape, offset, dtype):
    n, m = shape                                                 # n % 4 != 0: k_pdist<T, 1>; else <T, 4>
    pts, boxes = _scene(n, m, offset, dtype)
    rc, d, e, ok = _raw_forward(T(pts), T(boxes))
    assert rc == 0 and ok
    _check_forward(d, e, pts, boxes, dtype, "forward %s %s +%g" % (shape, dtype.__name__, offset))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", ref.OFFSETS)
def test_routes_agree_bit_for_bit(offset, dtype):
    """one problem with n % 4 == 0: aligned outputs take K = 4; dist moved on by one element and / or iedge by one byte take
    K = 1.  The same inlined function on the same operands: the same bits.  Without iedge (NULL) the distances stay."""
    n, m = 1024, 65
    pts, boxes = _scene(n, m, offset, dtype)
    tp, tb = T(pts), T(boxes)
    rc, d4, e4, ok = _raw_forward(tp, tb)
    assert rc == 0 and ok
    _check_forward(d4, e4, pts, boxes, dtype, "aligned %s +%g" % (dtype.__name__, offset))
    for sd, se in ((1, 1), (1, 0), (0, 1), (4, 2), (0, 4)):      # ((0, 4): both aligned again, K = 4 at another address)
        rc, d1, e1, ok = _raw_forward(tp, tb, shift_dist=sd, shift_iedge=se)
        assert rc == 0 and ok, (sd, se)
        assert np.array_equal(d1.view(np.uint8), d4.view(np.uint8)) and np.array_equal(e1, e4), (sd, se)
    for sd in (0, 1):
        rc, d0, _, ok = _raw_forward(tp, tb, shift_dist=sd, iedge=False)
        assert rc == 0 and ok and np.array_equal(d0.view(np.uint8), d4.view(np.uint8)), sd


def _mixed_boxes(dtype):
    """140 boxes, every other one with w or h in {0, -1.5, 0 and 0}: a row tile of 64 holds both kinds"""
    boxes = ref.scene(515, 140, 77, 0.0, np.float64)[1]
    odd = np.arange(1, 140, 2)
    for k, i in enumerate(odd):
        boxes[i, 2:4] = [(0, boxes[i, 3]), (boxes[i, 2], 0), (-1.5, boxes[i, 3]), (boxes[i, 2], -1.5), (0, 0)][k % 5]
    return boxes.astype(dtype), odd


@pytest.mark.parametrize("n", [515, 512])
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_positive_sizes(dtype, n):
    """w <= 0 or h <= 0: the forward kernel walks the edges as the reference does, zero-length edges included, and
    oracle.pdist2dr is the specification.  Values to the forward bound against the fp64 oracle on the same inputs; the
    regular rows between them as everywhere else; a degenerate row's feature must be one whose nearest point is as near as
    the best (coincident edges tie by rounding), and the one the model expects where the box has two sides of non-zero length."""
    boxes, odd = _mixed_boxes(dtype)
    pts = ref.scene(515, 140, 77, 0.0, dtype)[0][:n]
    rc, d, e, ok = _raw_forward(T(pts), T(boxes))
    assert rc == 0 and ok and not np.isnan(d).any() and (e < 8).all()
    p, b = _f64(pts), _f64(boxes)
    even = np.arange(0, 140, 2)
    _check_forward(d[even], e[even], pts, boxes[even], dtype, "regular rows among degenerate ones %s" % dtype.__name__)
    dref, eref = oracle.pdist2dr(p, b)
    tol = _value_tol(p, b, dtype)
    err = np.abs(d.astype(np.float64) - dref)
    print("degenerate %s n=%d: worst err / tol %.3f, features equal to the fp64 oracle's: %.4f" % (
        dtype.__name__, n, float((err / tol).max()), float((e[odd] == eref[odd]).mean())))
    assert (err <= tol).all()
    clear = np.abs(dref) > tol
    assert np.array_equal((d > 0)[clear], (dref > 0)[clear])
    feat, decided, accept = ref.features(p, b[odd], loop=True)
    decided &= ((b[odd, 2] != 0) & (b[odd, 3] != 0))[:, None]
    bad = ~ref.feature_ok(e[odd], feat, decided, accept)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert ref.feature_ok(eref[odd], feat, decided, accept).all()                # the oracle passes the same check


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_ties(dtype):
    """axis-aligned boxes of power-of-two sizes, points on a quarter-unit grid: on edges, corners, the centre, the diagonals
    and the extended sides every comparison is exact in both types.  Inside, the lower edge index wins a tie (geom.hpp
    point_box_distance_local; the reference's loop keeps the first minimum), so value and feature equal the oracle's."""
    boxes = np.array([[0, 0, 2, 2, 0], [0, 0, 4, 2, 0], [2, -1, 4, 2, 0], [-0.5, 0.25, 1, 4, 0]], dtype)
    ax = np.arange(-16, 17) / 4.0
    pts = np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2).astype(dtype)       # 1089 points: K = 1
    dref, eref = oracle.pdist2dr(pts, boxes)
    for n in (len(pts), 1088):                                                                # ... and K = 4
        rc, d, e, ok = _raw_forward(T(pts[:n]), T(boxes))
        assert rc == 0 and ok
        assert np.array_equal(d, dref[:, :n]) and np.array_equal(e, eref[:, :n]), n           # (-0.0 == 0.0)
    at = {tuple(p): j for j, p in enumerate(pts.tolist())}
    sq, wide = eref[0], eref[1]
    assert sq[at[(0.0, 0.0)]] == 0 and wide[at[(0.0, 0.0)]] == 0                              # four gaps tie; 0 and 2 tie
    assert [sq[at[q]] for q in ((0.5, -0.5), (0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5))] == [0, 1, 2, 0]      # the diagonals
    assert [sq[at[q]] for q in ((0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0))] == [0, 1, 2, 3]        # on the edges
    assert [sq[at[q]] for q in ((-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0))] == [4, 5, 6, 7]      # on the corners
    assert [sq[at[q]] for q in ((2.0, -1.0), (2.0, 1.0), (-1.0, 3.0), (-1.0, -3.0))] == [5, 6, 7, 4]      # on extended sides
    assert (dref[0][[at[q] for q in ((0.0, -1.0), (1.0, 1.0), (2.0, -1.0))]] == [0, 0, -1]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_and_refused(dtype):
    pts, boxes = _scene(5, 3, 0.0, dtype)
    for n, m in ((0, 3), (5, 0), (0, 0)):
        rc, d, e, ok = _raw_forward(T(pts), T(boxes), n=n, m=m)
        assert rc == 0 and ok and d.size == 0, (n, m)            # D3D_OK, and the whole buffer is still poison
    # one row tile more than a launch has: D3D_ERR_BAD_ARG before anything is written
    from d3d_amd import _lib
    m = 64 * 65535 + 1
    big = torch.ones((m, 5), dtype=T(boxes).dtype, device="cuda")
    rc, d, e, ok = _raw_forward(T(pts[:1]), big)
    assert rc == _lib.ERR_BAD_ARG and ok and np.isnan(d).all() and (e == 255).all()
    rc, gb, gp, ok, _ = _raw_backward(T(pts[:1]), big, torch.ones((m, 1), dtype=big.dtype, device="cuda"))
    assert rc == _lib.ERR_BAD_ARG and ok and np.isnan(gb).all() and np.isnan(gp).all()      # refused before it clears them


# ---------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def _bwd_case(n, m, offset, kind, dtype):
    pts, boxes, g, share = ref.backward_case(n, m, offset, kind, dtype)
    return (pts, boxes, g, share) + ref.grad_reference(_f64(pts), _f64(boxes), _f64(g))


@functools.lru_cache(maxsize=None)
def _cg32():
    """4 x the worst err / (eps * S) of the model itself in torch float32 on the CPU over the fp32 backward cases: one factor
    for the points and one per box parameter (the angle's is the largest: where one or two pairs weigh on a box, its lever
    arm can be a small part of the point's distance from the centre, to which the error is proportional)"""
    worst_p, worst_b = 0.0, np.zeros(5)
    for n, m in ref.BACKWARD_SHAPES:
        for offset in ref.OFFSETS:
            for kind in ref.WEIGHT_KINDS:
                pts, boxes, g, _, gp, gb, sp, sb = _bwd_case(n, m, offset, kind, np.float32)
                gp32, gb32, _, _ = ref.grad_reference(pts, boxes, g, torch.float32)
                rp = np.abs(gp32 - gp) / (EPS[np.float32] * np.where(sp > 0, sp, np.inf))
                rb = np.abs(gb32 - gb) / (EPS[np.float32] * np.where(sb > 0, sb, np.inf))
                worst_p, worst_b = max(worst_p, float(rp.max())), np.maximum(worst_b, rb.max(0))
    print("fp32 model err / (eps S): points %.3f, boxes %s" % (worst_p, np.round(worst_b, 3).tolist()))
    return 4 * worst_p, 4 * worst_b


@functools.lru_cache(maxsize=None)
def _cg64():
    """the same ratio for central differences of the fp64 oracle (as test_pdist_forward_backward takes them), or 64"""
    pts, boxes, g, _, gp, gb, sp, sb = _bwd_case(257, 65, 0.0, "dense", np.float64)
    h, worst = 1e-6, 0.0

    def loss(p, b):
        return float((oracle.pdist2dr(p, b)[0] * g).sum())
    for arr, ref_g, s, step in ((boxes, gb, sb, 13), (pts, gp, sp, 53)):
        for i in range(0, len(arr), step):
            for k in range(arr.shape[1]):
                a, c = arr.copy(), arr.copy()
                a[i, k] += h
                c[i, k] -= h
                fd = (loss(pts, a) - loss(pts, c)) / (2 * h) if arr is boxes else (loss(a, boxes) - loss(c, boxes)) / (2 * h)
                worst = max(worst, abs(fd - ref_g[i, k]) / (EPS[np.float64] * s[i, 0 if arr is pts else k]))
    print("central differences err / (eps S): %.3g" % worst)
    return min(worst, 64.0)


def _grad_bounds(dtype, sp, sb):
    cp, cb = _cg32() if dtype == np.float32 else (_cg64(), _cg64())
    tiny = float(np.finfo(dtype).tiny)
    return cp * EPS[dtype] * sp + tiny, cb * EPS[dtype] * sb + tiny


def _check_grads(gp, gb, case, dtype, tag):
    _, _, _, _, rp, rb, sp, sb = case
    bp, bb = _grad_bounds(dtype, sp, sb)
    ep, eb = np.abs(gp - rp), np.abs(gb - rb)
    print("%s: worst err / bound: points %.3f, boxes %.3f" % (tag, float((ep / bp).max()), float((eb / bb).max())))
    assert (ep <= bp).all(), (tag, np.argwhere(ep > bp)[:4].tolist())
    assert (eb <= bb).all(), (tag, np.argwhere(eb > bb)[:4].tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ref.WEIGHT_KINDS)
@pytest.mark.parametrize("offset", ref.OFFSETS)
@pytest.mark.parametrize("shape", ref.BACKWARD_SHAPES)
def test_backward_every_weight(shape, offset, kind, dtype):
    n, m = shape
    case = _bwd_case(n, m, offset, kind, dtype)
    pts, boxes, g, share = case[:4]
    assert share <= 0.01
    tag = "backward %s %s +%g %s" % (shape, dtype.__name__, offset, kind)
    tp, tb, tg = T(pts), T(boxes), T(g)
    rc, gb, gp, ok, outs = _raw_backward(tp, tb, tg)             # into NaN: whatever the entry does not clear shows
    assert rc == 0 and ok
    _check_grads(gp, gb, case, dtype, tag)
    rc, gb2, gp2, ok, _ = _raw_backward(tp, tb, tg, outs)        # into the first call's results: nothing carries over
    assert rc == 0 and ok
    _check_grads(gp2, gb2, case, dtype, tag + " (second call)")
    if kind == "zero_row_col":                                   # (exactly: no pair contributes)
        assert not gb[m // 2].any() and not gp[n // 3].any() and not gb2[m // 2].any() and not gp2[n // 3].any()
    if kind == "zero":
        assert not gb.any() and not gp.any()
    if kind == "sparse":
        assert not gb[~g.any(1)].any() and not gp[~g.any(0)].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_and_shim(dtype):
    """box2dr_pdist(...).backward() and box_impl's pdist2dr_backward in both argument orders hand out what the raw entry
    computes.  A point's gradient is two atomics onto zero here (65 boxes: two row tiles), and a + b == b + a: bit for
    bit.  A box's is one atomic per wavefront of points, five here, in any order: within one bound of the raw result."""
    from d3d_amd.box import box2dr_pdist, box_impl
    n, m = 257, 65
    case = _bwd_case(n, m, 50.0, "dense", dtype)
    pts, boxes, g = case[:3]
    rc, raw_b, raw_p, ok, _ = _raw_backward(T(pts), T(boxes), T(g))
    assert rc == 0 and ok
    _check_grads(raw_p, raw_b, case, dtype, "raw %s" % dtype.__name__)
    _, bound_b = _grad_bounds(dtype, case[6], case[7])

    def same_as_raw(gp, gb, tag):
        gp, gb = _f64(gp.cpu().numpy()), _f64(gb.cpu().numpy())
        assert gp.shape == (n, 2) and gb.shape == (m, 5), tag
        assert np.array_equal(gp, raw_p), tag
        assert (np.abs(gb - raw_b) <= bound_b).all(), tag

    tp, tb = T(pts).requires_grad_(True), T(boxes).requires_grad_(True)
    out = box2dr_pdist(tp, tb)
    rc, d, _, ok = _raw_forward(T(pts), T(boxes))
    assert rc == 0 and ok and np.array_equal(out.detach().cpu().numpy().view(np.uint8), d.view(np.uint8))
    out.backward(T(g))
    assert tp.grad.dtype == tp.dtype and tb.grad.dtype == tb.dtype
    same_as_raw(tp.grad, tb.grad, "autograd")
    for args in ((T(pts), T(boxes)), (T(boxes), T(pts))):
        gb, gp = box_impl.pdist2dr_backward(*args, T(g))
        same_as_raw(gp, gb, "shim")
        d2, _ = box_impl.pdist2dr_forward(*args)
        assert np.array_equal(d2.cpu().numpy().view(np.uint8), d.view(np.uint8))


# ---------------------------------------------------------------- box3dr_pdist
@functools.lru_cache(maxsize=None)
def _case3(axis):
    pts, boxes = ref.scene3(301, 40, axis, 300 + axis)
    kink = ref.kink_mask3(pts, boxes, axis)
    g = np.where(kink, 0.0, np.random.default_rng(310 + axis).random((40, 301)) - 0.3)
    return (pts, boxes, g, float(kink.mean()), ref.signed_distance3(pts, boxes, axis)) + ref.grad_reference3(pts, boxes, g, axis)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_box3dr_forward(axis):
    from d3d_amd.box import box3dr_pdist
    pts, boxes, _, _, model = _case3(axis)[:5]
    got = box3dr_pdist(T(pts), T(boxes), project_axis=axis).cpu().numpy()
    pc, bc = ref._AXES[axis]
    planar = ref.signed_distance(pts[:, pc], boxes[:, bc]) > 0
    along = np.abs(pts[None, :, axis] - boxes[:, axis, None]) < boxes[:, 3 + axis, None] / 2
    inside = (planar & along).any(0).mean()
    assert inside >= 0.25 and (planar & ~along).any(0).sum() > 30 and (~planar & along).any(0).sum() > 30
    err = np.abs(got - model) / (1e-12 * ref.scale3(pts, boxes))
    print("box3dr_pdist axis %d: worst err / tol %.3g, points inside a box %.2f" % (axis, float(err.max()), inside))
    assert got.shape == (40, 301) and (err <= 1).all()
    clear = np.abs(model) > 1e-9
    assert np.array_equal((got > 0)[clear], (planar & along)[clear])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_box3dr_backward(axis):
    from d3d_amd.box import box3dr_pdist
    pts, boxes, g, share, _, rp, rb, sp, sb = _case3(axis)
    assert share <= 0.01
    tp, tb = T(pts).requires_grad_(True), T(boxes).requires_grad_(True)
    box3dr_pdist(tp, tb, project_axis=axis).backward(T(g))
    bp, bb = _grad_bounds(np.float64, sp, sb)
    ep, eb = np.abs(tp.grad.cpu().numpy() - rp), np.abs(tb.grad.cpu().numpy() - rb)
    print("box3dr_pdist backward axis %d: excluded %.4f, worst err / bound: points %.3f, boxes %.3f" % (
        axis, share, float((ep / bp).max()), float((eb / bb).max())))
    assert (ep <= bp).all() and (eb <= bb).all()
