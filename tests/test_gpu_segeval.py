"""GPU: SegmentationEvaluator.calc_stats / calc_stats_batch (d3d_segeval) against the reference's goldens and the literal
restatement tests/seg_reference.py.  Integer counters exactly, cumiou to 1e-5 relative (the reference adds fp32 values in
hash-map order)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import seg_reference
from test_segeval import as_arrays, golden_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def stats_arrays(st):
    return as_arrays(st.as_object())


def check(ev, st, gl, pl, gi=None, pi=None, name=""):
    exp = seg_reference.calc_stats(ev._classes, ev._background, ev._min_points, gl, pl, gi, pi)
    c0, u0 = as_arrays(exp)
    c1, u1 = stats_arrays(st)
    assert np.array_equal(c1, c0), name
    np.testing.assert_allclose(u1, u0, rtol=1e-5, err_msg=name)
    return c1


def random_frame(rng, n, classes, nlab=12, nid=6):
    gl = rng.integers(0, nlab, n).astype(np.uint8)
    pl = np.where(rng.random(n) < 0.7, gl, rng.integers(0, nlab, n)).astype(np.uint8)
    gi = rng.integers(0, nid, n).astype(np.uint16)
    pi = np.where(rng.random(n) < 0.8, gi, rng.integers(0, nid, n)).astype(np.uint16)
    gl[:1] = 250                                                    # a gt label outside the classes (the background key)
    return gl, pl, gi, pi


def test_every_golden_case():
    from d3d_amd.benchmarks import SegmentationEvaluator
    for c in golden_cases():
        ev = SegmentationEvaluator(c["classes"], background=c["background"], min_points=c["min_points"])
        st = ev.calc_stats(c["gt_labels"], c["pred_labels"], c["gt_ids"], c["pred_ids"])
        counts, cum = stats_arrays(st)
        assert np.array_equal(counts, c["counts"]), c["name"]
        np.testing.assert_allclose(cum, c["cumiou"], rtol=1e-5, err_msg=c["name"])


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4097, 70001, 250000])
def test_seeded_random_frames_and_sizes(n):
    from d3d_amd.benchmarks import SegmentationEvaluator
    rng = np.random.default_rng(n)
    gl, pl, gi, pi = random_frame(rng, n, None)
    for mp in (0, 3):
        ev = SegmentationEvaluator([1, 2, 3, 5, 8, 11], background=0, min_points=mp)
        check(ev, ev.calc_stats(gl, pl), gl, pl, name="sem %d" % n)
        check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi, name="pano %d" % n)


def test_sub_tensor_views_at_odd_offsets():
    from d3d_amd.benchmarks import SegmentationEvaluator
    rng = np.random.default_rng(3)
    gl, pl, gi, pi = random_frame(rng, 20011, None)
    ev = SegmentationEvaluator([1, 2, 3, 4, 5], min_points=2)
    d = [torch.from_numpy(x).cuda() for x in (gl, pl, gi, pi)]
    for a, b in ((1, 20011), (3, 19000), (7, 9), (5, 4101)):
        views = [t[a:b] for t in d]
        assert views[0].data_ptr() % 16 != 0
        st = ev.calc_stats(*views)
        check(ev, st, gl[a:b], pl[a:b], gi[a:b], pi[a:b], name="view %d:%d" % (a, b))
    # labels aligned, ids not (the vector path needs all four)
    st = ev.calc_stats(d[0][16:], d[1][16:], d[2][15:-1], d[3][14:-2])
    check(ev, st, gl[16:], pl[16:], gi[15:-1], pi[14:-2])


def test_all_background_and_labels_outside_the_classes():
    from d3d_amd.benchmarks import SegmentationEvaluator
    ev = SegmentationEvaluator([1, 2], background=0)
    z = np.zeros((5000,), np.uint8)
    ids = np.arange(5000).astype(np.uint16)
    c = check(ev, ev.calc_stats(z, z, ids, ids), z, z, ids, ids)
    assert c.sum() == 0
    out = np.full((5000,), 77, np.uint8)                             # labels that are not classes: background keys
    c = check(ev, ev.calc_stats(out, z, ids, ids), out, z, ids, ids)
    assert c.sum() == 0
    gl = np.where(np.arange(5000) % 3 == 0, 1, 77).astype(np.uint8)
    pl = np.where(np.arange(5000) % 2 == 0, 2, 99).astype(np.uint8)
    c = check(ev, ev.calc_stats(gl, pl, ids, ids), gl, pl, ids, ids)
    assert c[2, 1] == 1667 and c[1, 2] == 2500 and c[5, 1] == 1667 and c[4, 2] == 2500


def test_label_255_with_ids_0_and_65535():
    from d3d_amd.benchmarks import SegmentationEvaluator
    n = 4000
    gl = np.full((n,), 255, np.uint8)
    gl[:7] = 3                                                       # background keys present
    gi = np.where(np.arange(n) % 2 == 0, 0, 65535).astype(np.uint16)
    pl = gl.copy()
    pi = gi.copy()
    pi[::10] ^= 0xffff
    for bg in (0, 3):
        ev = SegmentationEvaluator([255, 3], background=bg)
        c = check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)
        assert c[3, 255] == 2
    ev = SegmentationEvaluator([255, 3], background=-1)              # 255 is the background: nothing for it
    c = check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)
    assert c[:, 255].sum() == 0


def test_min_points_at_the_segment_size_and_one_above():
    from d3d_amd.benchmarks import SegmentationEvaluator
    seg = 37
    gl = np.concatenate([[9], np.full((seg,), 1)]).astype(np.uint8)
    gi = np.concatenate([[0], np.full((seg,), 4)]).astype(np.uint16)
    pl, pi = gl.copy(), gi.copy()
    pi[-1] = 5                                                       # pred 1|4: seg - 1 points, pred 1|5: one point
    for mp, matched in ((seg, 1), (seg + 1, 0)):
        ev = SegmentationEvaluator([1, 2], min_points=mp)
        c = check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)
        assert c[3, 1] == matched and c[5, 1] == 0                   # gt 1|4 (seg points) takes part at seg, not at seg + 1
        assert c[4, 1] == 0                                          # both predictions are below min_points
    ev = SegmentationEvaluator([1, 2], min_points=1)
    c = check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)
    assert c[3, 1] == 1 and c[4, 1] == 1                              # pred 1|5 (1 point) is a false positive segment at 1
    ev = SegmentationEvaluator([1, 2], min_points=2)
    c = check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)
    assert c[3, 1] == 1 and c[4, 1] == 0                              # ... and not at 2


def test_iou_exactly_one_half_does_not_match():
    from d3d_amd.benchmarks import SegmentationEvaluator
    # gt 1|1: 6 points, pred 1|2: 6 points, 4 shared -> 4 / (6 + 6 - 4) = 0.5
    gl = np.array([7] + [1] * 8, np.uint8)
    gi = np.array([0, 1, 1, 1, 1, 1, 1, 3, 3], np.uint16)
    pl = np.array([7] + [1] * 8, np.uint8)
    pi = np.array([0, 2, 2, 2, 2, 4, 4, 2, 2], np.uint16)
    ev = SegmentationEvaluator([1])
    c = check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)
    assert c[3, 1] == 0 and c[5, 1] == 2 and c[4, 1] == 2
    pi[6] = 2                                                        # inter 5 / (6 + 7 - 5) = 0.625
    c = check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)
    assert c[3, 1] == 1


def test_every_point_of_a_valid_class():
    """no point carries the background key: the reference's counter[bg_key] then inserts into the map it iterates (UB);
    the GPU path defines union = g + p - inter, the checker's reading"""
    from d3d_amd.benchmarks import SegmentationEvaluator
    rng = np.random.default_rng(11)
    n = 30000
    gl = rng.integers(1, 6, n).astype(np.uint8)
    gi = rng.integers(0, 4, n).astype(np.uint16)
    pl = np.where(rng.random(n) < 0.9, gl, rng.integers(1, 6, n)).astype(np.uint8)
    pi = gi.copy()
    ev = SegmentationEvaluator([1, 2, 3, 4, 5])
    c = check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)
    assert c[3].sum() > 0


def test_more_distinct_pairs_than_the_lds_table():
    from d3d_amd.benchmarks import SegmentationEvaluator
    rng = np.random.default_rng(5)
    n = 40000                                                        # ~4096 distinct pairs per workgroup > 2048 LDS slots
    gl = rng.integers(1, 4, n).astype(np.uint8)
    gi = rng.integers(0, 65536, n).astype(np.uint16)
    pl = gl.copy()
    pi = np.where(rng.random(n) < 0.5, gi, rng.integers(0, 65536, n)).astype(np.uint16)
    gl[0] = 200
    for mp in (0, 1, 2):
        ev = SegmentationEvaluator([1, 2, 3], min_points=mp)
        check(ev, ev.calc_stats(gl, pl, gi, pi), gl, pl, gi, pi)


def test_batch_equals_per_frame_calls():
    from d3d_amd import synth
    from d3d_amd.benchmarks import SegmentationEvaluator
    sizes = [0, 1, 17, 4096, 0, 30000, 5, 120000, 0]
    frames = [synth.segmentation_frame(s, num_classes=6, inst_per_class=4, noise=0.2, seed=i) for i, s in enumerate(sizes)]
    cat = [np.concatenate([f[k] for f in frames]) for k in range(4)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    for mp in (0, 10):
        ev = SegmentationEvaluator([1, 2, 3, 4, 6], min_points=mp)
        for ids in (False, True):
            b = ev.calc_stats_batch(cat[0], cat[1], cat[2] if ids else None, cat[3] if ids else None, off)
            assert len(b) == len(sizes)
            for f, st in zip(frames, b):
                one = ev.calc_stats(f[0], f[1], f[2], f[3]) if ids else ev.calc_stats(f[0], f[1])
                assert st == one
                check(ev, st, *(f if ids else f[:2]))
    ev = SegmentationEvaluator([1])
    assert ev.calc_stats_batch(cat[0][:0], cat[1][:0], frame_offsets=[0]) == []
    with pytest.raises(ValueError):
        ev.calc_stats_batch(cat[0], cat[1], frame_offsets=[0, 5, 3, len(cat[0])])
    with pytest.raises(ValueError):
        ev.calc_stats_batch(cat[0], cat[1], frame_offsets=[0, 5])


def test_device_tensors_in_equal_numpy_in_and_runs_are_bit_identical():
    from d3d_amd import synth
    from d3d_amd.benchmarks import SegmentationEvaluator
    gl, pl, gi, pi = synth.segmentation_frame(300000, seed=4)
    ev = SegmentationEvaluator(list(range(1, 20)), min_points=5)
    a = ev.calc_stats(gl, pl, gi, pi)
    d = [torch.from_numpy(x).cuda() for x in (gl, pl, gi, pi)]
    b = ev.calc_stats(*d)
    c = ev.calc_stats(*d)
    assert a == b == c
    assert all(np.float32(a.cumiou[k]).tobytes() == np.float32(c.cumiou[k]).tobytes() for k in a.cumiou)
    assert sum(a.itp.values()) > 100
    check(ev, a, gl, pl, gi, pi)
    with pytest.raises(ValueError, match="uint16"):
        ev.calc_stats(d[0], d[1], d[2].to(torch.int32), d[3])


def raw_call(gl, pl, gi, pi, off, classes, bg, mp, out, ws, wsb):
    from d3d_amd import _lib
    lib = _lib.load()
    mask = (ctypes.c_uint32 * 8)()
    for c in classes:
        mask[c >> 5] |= 1 << (c & 31)
    rows = [_lib.ptr(out[k]) for k in range(7)]
    return lib.d3d_segeval(_lib.ptr(gl), _lib.ptr(pl), _lib.ptr(gi) if gi is not None else None,
                           _lib.ptr(pi) if pi is not None else None, _lib.ptr(off), gl.numel(), off.numel() - 1, mask, bg, mp,
                           *rows, _lib.ptr(ws), wsb, None)


def test_raw_c_entry_with_its_workspace_query_and_poisoned_outputs():
    from d3d_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(9)
    sizes = [1000, 0, 2500, 64]
    frames = [random_frame(rng, s, None) for s in sizes]
    cat = [torch.from_numpy(np.concatenate([f[k] for f in frames])).cuda() for k in range(4)]
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device="cuda")
    F, n = len(sizes), int(sum(sizes))
    wsb = lib.d3d_segeval_workspace_bytes(n, F)
    ws = torch.full((wsb,), 0x5a, dtype=torch.uint8, device="cuda")            # dirty scratch
    classes, bg, mp = [0, 1, 2, 4, 7], 0, 2
    for pano in (False, True):
        out = torch.full((7, F, 256), -12345, dtype=torch.int32, device="cuda")     # poisoned results
        st = raw_call(cat[0], cat[1], cat[2] if pano else None, cat[3] if pano else None, off, classes, bg, mp, out, ws, wsb)
        assert st == _lib.OK
        res = out.cpu().numpy()
        cum = res[6].view(np.float32)
        for f, fr in enumerate(frames):
            exp = seg_reference.calc_stats(classes, bg, mp, *(fr if pano else fr[:2]))
            counts, u = as_arrays(exp)
            assert np.array_equal(res[:6, f], counts), (pano, f)
            np.testing.assert_allclose(cum[f], u, rtol=1e-5)
    assert raw_call(cat[0], cat[1], cat[2], cat[3], off, classes, bg, mp, out, ws, wsb - 256) == _lib.ERR_WORKSPACE
    assert raw_call(cat[0], cat[1], cat[2], None, off, classes, bg, mp, out, ws, wsb) == _lib.ERR_BAD_ARG
    torch.cuda.synchronize()
