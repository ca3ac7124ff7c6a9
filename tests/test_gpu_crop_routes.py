"""The point-in-box kernels of crop.hip and k_crop2dr of box.hip on every launch route and every level of the box grid, bit for
bit against the CPU oracle (oracle.crop_points, paint_label, crop_2dr, box3dp_crop) on the scenes of tests/crop_cases.py
(tests/test_crop_cases.py holds those scenes against the oracle without a GPU).  No mismatch budget anywhere.

What each test reaches that the suite did not:
  test_grid_levels                k_crop3dr_grid, k_paint_label_grid, k_crop2dr_grid, k_crop3dp_grid at 32, 16 and 8 cells per axis
                                  and on G.all, each level through every way that leads to it; one workgroup exactly, a second
                                  one with a single point, n % 4 != 0; points on, one fp32 step outside and far outside the
                                  boxes' common range; NaN / inf points; the memset of the grid routes (poisoned outputs);
                                  box3dp_crop against the oracle instead of against crop_2dr, which shares its grid
  test_all_pairs_kernels          k_crop3dr, k_paint_label, k_crop2dr<float>, k_crop2dr<double>: blockIdx.y > 0, full and partial
                                  last tile, word and byte stores, a last workgroup with idle lanes, the lowest index across
                                  tiles, the early exit, a match in the last tile only, m > 4096 with n >= 4096
  test_routes_agree               the grid route's columns against the all-pairs kernels on pieces of 4095 points
  test_box3dp_crop_every_axis     axes 0 and 1 by VALUE (they were checked for their shape), fp32 and fp64
  test_empty_refused_and_wrapped  m == 0 on both routes, n == 0, uint16 ids beyond 65535 boxes, more than 65535 box tiles
  test_misaligned_output          the C ABI with an `out` one byte off a word: guard bytes on both sides

The plan of every scene, as d3d_internal_box_grid_plan reports it from the production build_box_grid (PLANS below;
{cells per axis, G.all, registrations}; the same for [M,7], [M,9], stride-11 rows and the (x, y, w, h, r) rows of crop_2dr):
  g32          {32, 0, 1127}    200 boxes of 1.5 - 5.5 m
  g16_list     {16, 0, 5621}    2000 such boxes: 11143 registrations at 32
  g16_box      {16, 0,  595}    g32 and one 30 x 30 m box, yaw 0.3: more than 64 cells at 32
  g8_box       { 8, 0,  377}    g32 and one 60 x 60 m box: more than 64 cells at 32 and at 16
  g8_single    { 8, 0,   64}    one box: the grid spans the box, which covers every cell of every level
  all_list     { 0, 1,    0}    1000 boxes of 25 - 30 m: 9181 registrations at 8
  all_nan, all_inf_w, all_inf_yaw
               { 0, 1,    0}    g32 with a NaN centre, an infinite width, an infinite yaw in row 57
  zero_extent  {32, 0,    5}    five boxes of no width at one place: the range is a point, ix = iy = 0, every box in cell 0
  huge_extent  {32, 0,   52}    hi - lo = inf in x: ix = 0, a finite distance lands in column 0 and an infinite one (inf * 0 =
                                NaN, which fminf drops for n - 1) in column 31; both boxes and every point follow the same map

What changed beside the tests: k_crop3dr and k_crop2dr chose their 32-bit store from n % 4 == 0 alone; with an `out` that is
not 4-byte aligned (the C ABI takes any address) every row store was a misaligned word.  They now look at the pointer too, as
the pdist kernels do (test_misaligned_output).  Non-finite box rows: a row with a NaN centre, an infinite width or an infinite
yaw holds no point for the oracle (every comparison with NaN fails; inf - inf in the edge functions), the reference's
dgal_wrap.h:6-19 makes the same comparisons, and both routes of every operator agree with it.  Nothing else was found: all
88 cases passed on the kernels as they were.

One-line reversions tried against these tests on an MI355X (each on a copy of the library): without the i0 tile offset in
k_crop3dr's output row 24 cases fail (every all-pairs case with m > 64, test_routes_agree on every scene of more than 64
boxes); with k_paint_label walking a tile's rows downwards 27 fail; with `<` for `<=` in the cell columns of build_box_grid
(count and fill alike, so that the lists stay consistent) 32 fail, among them every level-8 scene, zero_extent and
huge_extent.  The G.all assignment at gn == 8 was NOT removed on a device: all_list would then fill 9181 entries into the
8192-entry list in LDS; its asserted plan {0, 1, 0} is what holds that line."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import crop_cases as cc
import oracle

pytestmark = pytest.mark.gpu

PLANS = {"g32": [32, 0, 1127, 0], "g16_list": [16, 0, 5621, 0], "g16_box": [16, 0, 595, 0], "g8_box": [8, 0, 377, 0],
         "g8_single": [8, 0, 64, 0], "all_list": [0, 1, 0, 0], "all_nan": [0, 1, 0, 0], "all_inf_w": [0, 1, 0, 0],
         "all_inf_yaw": [0, 1, 0, 0], "zero_extent": [32, 0, 5, 0], "huge_extent": [32, 0, 52, 0]}
POISON = 0xAB
B5 = [0, 1, 3, 4, 6]            # (x, y, w, h, r) of a 7-float row


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


@functools.lru_cache(maxsize=None)
def _L():
    from d3d_amd import _lib
    lib = _lib.load()
    lib.d3d_internal_box_grid_plan.restype = ctypes.c_int
    lib.d3d_internal_box_grid_plan.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_void_p, ctypes.c_void_p]
    return _lib, lib


def probe(rows, offset, dims):
    _lib, lib = _L()
    plan = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    rc = lib.d3d_internal_box_grid_plan(P(rows), rows.shape[0], rows.shape[1], offset, dims, P(plan), _lib.stream_ptr())
    return rc, plan.cpu().tolist()


# the raw entries on poisoned outputs: every byte of the result is the kernels' (or their memset's) own
def raw_crop3dr(pts, rows, offset):
    _lib, lib = _L()
    m, n = rows.shape[0], pts.shape[0]
    out = torch.full((m, n), POISON, dtype=torch.uint8, device="cuda")
    rc = lib.d3d_crop_3dr(P(pts), n, pts.shape[1], P(rows), m, rows.shape[1], offset, P(out), _lib.stream_ptr())
    assert rc == _lib.OK
    return out


def raw_paint(pts, sem, rows, offset, labels):
    _lib, lib = _L()
    m, n = rows.shape[0], pts.shape[0]
    ids = torch.full((n,), POISON * 257 - 65536, dtype=torch.int16, device="cuda")
    rc = lib.d3d_paint_label(P(pts), n, pts.shape[1], P(sem), P(rows), m, rows.shape[1], offset, P(labels), P(ids), _lib.stream_ptr())
    assert rc == _lib.OK
    return ids


def raw_crop2dr(pts2, b5):
    _lib, lib = _L()
    m, n = b5.shape[0], pts2.shape[0]
    out = torch.full((m, n), POISON, dtype=torch.uint8, device="cuda")
    code = _lib.F64 if pts2.dtype == torch.float64 else _lib.F32
    assert lib.d3d_crop_2dr(P(pts2), n, P(b5), m, code, P(out), _lib.stream_ptr()) == _lib.OK
    return out


def raw_crop3dp(pts, b7):
    _lib, lib = _L()
    m, n = b7.shape[0], pts.shape[0]
    out = torch.full((m, n), POISON, dtype=torch.uint8, device="cuda")
    assert lib.d3d_crop_3dp(P(pts), n, pts.shape[1], P(b7), m, 7, 2, P(out), _lib.stream_ptr()) == _lib.OK
    return out


def u16(ids):
    return ids.cpu().numpy().astype(np.int64).astype(np.uint16) if ids.dtype != torch.int16 else ids.cpu().numpy().view(np.uint16)


def same(got, exp):
    """array_equal on the BYTES: a bool mask is 0 / 1, nothing of the poison left"""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return np.array_equal(got.view(np.uint8), np.asarray(exp).view(np.uint8))


def expected(sc):
    with np.errstate(all="ignore"):
        return (oracle.crop_points(sc.boxes, sc.pts), oracle.paint_label(sc.rows9, sc.pts, sc.sem),
                oracle.crop_2dr(sc.pts[:, :2].copy(), sc.boxes[:, B5].copy()), oracle.box3dp_crop(sc.pts[:, :3], sc.boxes, 2))


@pytest.mark.parametrize("n", [4096, 4097, 8191])
@pytest.mark.parametrize("name", cc.SCENES)
def test_grid_levels(name, n):
    from d3d_amd.abstraction import crop_points, paint_label
    from d3d_amd.box import box3dp_crop, crop_2dr
    _lib, _ = _L()
    sc = cc.scene(name, n)
    b7, b9, b11, b5 = T(sc.boxes), T(sc.rows9), T(cc.rows11(sc.boxes)), T(sc.boxes[:, B5])
    plans = [probe(b7, 0, 3), probe(b9, 2, 3), probe(b11, 3, 3), probe(b5, 0, 2)]
    print(name, n, plans[0][1])
    assert plans == [(_lib.OK, PLANS[name])] * 4
    e3, eid, e2, ep = expected(sc)
    p6, p4, p3, p2 = T(sc.pts), T(sc.pts[:, :4]), T(sc.pts[:, :3]), T(sc.pts[:, :2])
    sem, lab = T(sc.sem), T(sc.labels)
    assert same(raw_crop3dr(p6, b11, 3), e3)
    assert same(crop_points(b7, p3), e3) and same(crop_points(b9, p4), e3)
    assert np.array_equal(u16(raw_paint(p6, sem, b11, 3, lab)), eid)
    assert np.array_equal(u16(paint_label(b9, p4, sem)), eid) and np.array_equal(u16(paint_label(b7, p3, sem, labels=lab)), eid)
    assert same(raw_crop2dr(p2, b5), e2) and same(crop_2dr(p2, b5), e2)
    assert same(raw_crop3dp(p6, b7), ep)
    assert same(box3dp_crop(p3, b7, 2), ep) and same(box3dp_crop(p6, b7), ep)


ALL_PAIRS = [(m, n) for m in (1, 63, 64, 65, 129) for n in (1, 3, 4, 1023, 1024, 1025, 4095)] + [(4097, 4096), (4097, 4099)]


def _all_pairs(sc):
    """the four all-pairs kernels on a scene with n < 4096 or m > 4096, raw entries, poisoned outputs"""
    odd = sc.m % 2 == 1                                     # both row layouts over the cases
    rows, off = (T(cc.rows11(sc.boxes)), 3) if odd else (T(sc.boxes), 0)
    pts = T(sc.pts) if odd else T(sc.pts[:, :3])
    with np.errstate(all="ignore"):
        assert same(raw_crop3dr(pts, rows, off), oracle.crop_points(sc.boxes, sc.pts))
        assert np.array_equal(u16(raw_paint(pts, T(sc.sem), rows, off, T(sc.labels))),
                              oracle.paint_label(sc.boxes, sc.pts, sc.sem, labels=sc.labels))
        for dt in (np.float32, np.float64):
            p2, b5 = sc.pts[:, :2].astype(dt), sc.boxes[:, B5].astype(dt)
            assert same(raw_crop2dr(T(p2), T(b5)), oracle.crop_2dr(p2, b5)), dt


@pytest.mark.parametrize("m,n", ALL_PAIRS)
def test_all_pairs_kernels(m, n):
    _all_pairs(cc.pairs_scene(m, n))
    if (m, n) == (129, 1025):
        for sc in (cc.paint_early_exit(), cc.paint_last_tile()):
            exp = oracle.paint_label(sc.boxes, sc.pts, sc.sem, labels=sc.labels)
            assert np.array_equal(u16(raw_paint(T(sc.pts), T(sc.sem), T(sc.boxes), 0, T(sc.labels))), exp)
        assert np.all(exp == 129)                           # (the last one: the only match is in the last tile)


@pytest.mark.parametrize("name", cc.SCENES)
def test_routes_agree(name):
    """the grid kernels (n = 8191) against the all-pairs kernels (pieces of 4095 points), GPU against GPU: holds whatever the
    oracle makes of a non-finite row"""
    from d3d_amd.box import box3dp_crop, crop_2dr
    n, piece = 8191, 4095
    sc = cc.scene(name, n)
    b7, b9, b5, sem, lab = T(sc.boxes), T(sc.rows9), T(sc.boxes[:, B5]), T(sc.sem), T(sc.labels)
    p6 = T(sc.pts)
    g3, gid = raw_crop3dr(p6, b9, 2), raw_paint(p6, sem, b9, 2, lab)
    g2, gp = raw_crop2dr(p6[:, :2].contiguous(), b5), raw_crop3dp(p6, b7)
    for j0 in range(0, n, piece):
        q6, s = p6[j0:j0 + piece].contiguous(), sem[j0:j0 + piece].contiguous()
        assert q6.shape[0] < 4096
        assert torch.equal(raw_crop3dr(q6, b9, 2), g3[:, j0:j0 + piece])
        assert torch.equal(raw_paint(q6, s, b9, 2, lab), gid[j0:j0 + piece])
        assert torch.equal(raw_crop2dr(q6[:, :2].contiguous(), b5), g2[:, j0:j0 + piece])
        assert torch.equal(box3dp_crop(q6[:, :3].contiguous(), b7, 2).view(torch.uint8), gp[:, j0:j0 + piece])
        assert torch.equal(crop_2dr(q6[:, :2].contiguous(), b5).view(torch.uint8), g2[:, j0:j0 + piece])


@pytest.mark.parametrize("n", [1003, 5000])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box3dp_crop_every_axis(dtype, n):
    """axes 0 and 1: the composition around crop_2dr (fp32 with n >= 4096: k_crop2dr_grid on (x, y, w, h, r) rows; otherwise
    k_crop2dr); axis 2 in fp32 with n >= 4096: the one launch"""
    from d3d_amd.box import box3dp_crop
    pts, boxes = cc.axes_scene(n, dtype)
    for ax in (0, 1, 2):
        exp = oracle.box3dp_crop(pts, boxes, ax)
        assert exp.any(0).sum() >= 0.1 * n
        got = box3dp_crop(T(pts), T(boxes), ax)
        assert got.dtype == torch.bool and same(got, exp), ax


def test_empty_refused_and_wrapped():
    from d3d_amd.abstraction import crop_points, paint_label
    _lib, lib = _L()
    st = _lib.stream_ptr()
    sc = cc.scene("g32", 5000)
    none7 = torch.empty((0, 7), dtype=torch.float32, device="cuda")
    guard = torch.full((64,), POISON, dtype=torch.uint8, device="cuda")
    for n in (100, 5000):                                   # m == 0: all-pairs and grid route
        p, s = T(sc.pts[:n]), T(sc.sem[:n])
        assert not u16(raw_paint(p, s, none7, 0, None)).any()
        assert not u16(paint_label(none7, p, s, labels=torch.empty((0,), dtype=torch.uint8, device="cuda"))).any()
        assert lib.d3d_crop_3dr(P(p), n, 6, None, 0, 7, 0, P(guard), st) == _lib.OK
        assert lib.d3d_crop_3dp(P(p), n, 6, None, 0, 7, 2, P(guard), st) == (_lib.OK if n >= 4096 else _lib.ERR_UNSUPPORTED)
        assert lib.d3d_crop_2dr(P(p), n, None, 0, _lib.F32, P(guard), st) == _lib.OK
        assert crop_points(none7, p).shape == (0, n)
    b7, lab = T(sc.boxes), T(sc.labels)                     # n == 0
    assert lib.d3d_crop_3dr(None, 0, 3, P(b7), sc.m, 7, 0, P(guard), st) == _lib.OK
    assert lib.d3d_paint_label(None, 0, 3, None, P(b7), sc.m, 7, 0, P(lab), P(guard), st) == _lib.OK
    assert lib.d3d_crop_2dr(None, 0, P(b7), sc.m, _lib.F32, P(guard), st) == _lib.OK
    none3 = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    assert crop_points(b7, none3).shape == (sc.m, 0)
    assert paint_label(b7, none3, torch.empty((0,), dtype=torch.uint8, device="cuda"), labels=lab).shape == (0,)
    assert bool((guard == POISON).all())
    # ids beyond uint16: wrapped as the reference's uint16 array wraps them
    w = cc.wrap_scene()
    exp = oracle.paint_label(w.boxes, w.pts, w.sem, labels=w.labels)
    assert np.all(exp[w.sem == 3] == 0) and np.all(exp[w.sem == 4] == 5) and w.m > 65535
    assert np.array_equal(u16(raw_paint(T(w.pts), T(w.sem), T(w.boxes), 0, T(w.labels))), exp)
    assert np.array_equal(u16(paint_label(T(w.boxes), T(w.pts), T(w.sem), labels=T(w.labels))), exp)
    # more box tiles than a launch has rows of workgroups: refused, nothing written
    m = 65535 * 64 + 1
    boxes = torch.zeros((m, 7), dtype=torch.float32, device="cuda")
    out, one = torch.full((m,), POISON, dtype=torch.uint8, device="cuda"), T(sc.pts[:1])
    assert lib.d3d_crop_3dr(P(one), 1, 6, P(boxes), m, 7, 0, P(out), st) == _lib.ERR_BAD_ARG
    assert bool((out == POISON).all())
    assert probe(torch.zeros((4097, 7), dtype=torch.float32, device="cuda"), 0, 3)[0] == _lib.ERR_UNSUPPORTED
    assert probe(none7, 0, 3) == (_lib.OK, [0, 1, 0, 0])    # no box: G.all, a loop over nothing


@pytest.mark.parametrize("m,n", [(65, 1024), (65, 4096)])
def test_misaligned_output(m, n):
    """`out` one byte past a word boundary with n % 4 == 0: rows of bytes, not of words (all-pairs kernels; the grid routes
    store bytes and clear with a memset), and nothing outside [out, out + m * n)"""
    _lib, lib = _L()
    st = _lib.stream_ptr()
    sc = cc.pairs_scene(m, n)
    front = 65
    for what in ("3dr", np.float32, np.float64):
        buf = torch.full((front + m * n + 64,), POISON, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        out = ctypes.c_void_p(buf.data_ptr() + front)
        if what == "3dr":
            p, b = T(sc.pts), T(sc.boxes)                   # (named: they must outlive the launch)
            rc = lib.d3d_crop_3dr(P(p), n, 6, P(b), m, 7, 0, out, st)
            exp = oracle.crop_points(sc.boxes, sc.pts)
        else:
            p2, b5 = sc.pts[:, :2].astype(what), sc.boxes[:, B5].astype(what)
            p, b = T(p2), T(b5)
            rc = lib.d3d_crop_2dr(P(p), n, P(b), m, _lib.F64 if what is np.float64 else _lib.F32, out, st)
            exp = oracle.crop_2dr(p2, b5)
        assert rc == _lib.OK
        got = buf.cpu().numpy()
        assert np.all(got[:front] == POISON) and np.all(got[front + m * n:] == POISON)
        assert np.array_equal(got[front:front + m * n].reshape(m, n), exp.view(np.uint8)), what
