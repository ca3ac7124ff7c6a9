"""The refusals of the box, matcher and transform fronts, word for word and with the exception type: everything here answers on the
host, before the library is loaded and before a GPU is asked for (what answers later is in test_gpu_box_front.py).  With two faults
in one call the order of the checks is part of the interface too.  Then the rules the Python layer keeps after these fronts moved
onto shared helpers -- one definition of each message, of the host conversion and of the threshold lookup, no offset arithmetic on a
shipped buffer -- and the threshold lookup against the three spellings it replaced.
"""
import os
import re

import numpy as np
import pytest
import torch

from d3d_amd import _lib, box
from d3d_amd.tracking import matcher

MIXED = "Input should be both numpy tensor or pytorch tensor!"
NX2 = "Input of rbox_2d_iou should be Nx2 tensors!"
F5 = "Input boxes should have 5 fields: x, y, w, h, r"
F7 = "Input boxes should have 7 fields: x, y, z, lx, ly, lz, rz"
AXIS = "The projection axis can only be 0-x, 1-y and 2-z!"
SAME = "boxes1 and boxes2 must have the same dtype"
FLOATS = "boxes must be float32 or float64"
ROWS9 = "%s should be [n,9] rows of (label, score, x, y, z, lx, ly, lz, yaw)"
HARD = "box2d_nms_batched does hard NMS only: soft-NMS is sequential per set, use box2d_nms on each group"


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def refused(exc, message, fn, *args, **kw):
    with pytest.raises(exc) as e:
        fn(*args, **kw)
    assert type(e.value) is exc
    if message is not None:
        assert str(e.value) == message


FIVE = (box.box2d_iou, box.box2d_iou_paired, box.box2d_iou_sparse)            # fronts on [N,5] rows
SEVEN = (box.box3d_iou_paired, box.iou3d_sparse)                              # fronts on [N,7] rows that check before loading


def test_numpy_mixed_with_torch():
    for fn in FIVE:
        refused(AssertionError, MIXED, fn, np.zeros((3, 5)), z(3, 5))
    for fn in SEVEN:
        refused(AssertionError, MIXED, fn, np.zeros((3, 7)), z(3, 7))
    refused(AssertionError, MIXED, box.box2d_nms, np.zeros((3, 5)), z(3))
    refused(AssertionError, MIXED, box.box2d_nms_batched, np.zeros((3, 5)), z(3), np.zeros(3, np.int64))


def test_row_shapes():
    for fn in FIVE:
        refused(ValueError, NX2, fn, z(5), z(3, 5))
        refused(ValueError, NX2, fn, z(3, 5), z(3, 5, 1))
        for cols in (4, 6):
            refused(ValueError, F5, fn, z(3, cols), z(3, 5))
            refused(ValueError, F5, fn, z(3, 5), z(3, cols))
            refused(ValueError, F5, fn, np.zeros((3, 5)), np.zeros((3, cols)))
    for fn in SEVEN:
        refused(ValueError, F7, fn, z(7), z(3, 7))                            # (one combined condition: no message for the rank)
        refused(ValueError, F7, fn, z(3, 7), z(7))
        for cols in (6, 8):
            refused(ValueError, F7, fn, z(3, cols), z(3, 7))
            refused(ValueError, F7, fn, z(3, 7), z(3, cols))
    refused(ValueError, "Input boxes should be Nx2 tensors!", box.box2dr_pdist, z(4, 2), z(5))
    for cols in (4, 6):
        refused(ValueError, F5, box.box2dr_pdist, z(4, 2), z(3, cols))
    refused(ValueError, "Only supported rotated boxes by now!", box.box2dr_pdist, z(4, 2), z(3, 5), method="box")


def test_pair_counts():
    refused(ValueError, "Paired boxes should come in equal numbers: 3 and 4", box.box2d_iou_paired, z(3, 5), z(4, 5))
    refused(ValueError, "Paired boxes should come in equal numbers: 4 and 3", box.box3d_iou_paired, z(4, 7), z(3, 7))


def test_method_names():
    for fn in FIVE:
        with pytest.raises(AttributeError, match="CIRCLE"):
            fn(z(3, 5), z(3, 5), method="circle")
    for method in ("na", "gbox", "dbox"):                                     # names of the enum without a function
        refused(ValueError, "Unrecognized iou type!", box.box2d_iou, z(3, 5), z(3, 5), method=method)
        refused(ValueError, "Unrecognized iou type!", box.box2d_iou_paired, z(3, 5), z(3, 5), method=method)
    for method in ("grbox", "drbox", "na"):
        refused(ValueError, "Unsupported iou type!", box.box2d_iou_sparse, z(3, 5), z(3, 5), method=method)
        refused(ValueError, "Unsupported iou type!", box.iou3d_sparse, z(3, 7), z(3, 7), method=method)
        refused(ValueError, "Unrecognized iou type!", box.box3d_iou_paired, z(3, 7), z(3, 7), method=method)
    refused(ValueError, "Unrecognized iou type!", box.iou3d_sparse, z(3, 7), z(3, 7), method="circle")
    refused(ValueError, "Unrecognized iou type!", box.box3d_iou_paired, z(3, 7), z(3, 7), method="circle")


@pytest.mark.parametrize("bad", [float("nan"), -1, float("inf"), "x", None])
def test_sparse_threshold(bad):
    message = "threshold should be a finite number >= 0, got %r" % (bad,)
    refused(ValueError, message, box.box2d_iou_sparse, z(3, 5), z(3, 5), threshold=bad)
    refused(ValueError, message, box.iou3d_sparse, z(3, 7), z(3, 7), threshold=bad)


def test_dtypes_of_the_paired_and_sparse_fronts():
    for fn in (box.box2d_iou_paired, box.box2d_iou_sparse):
        refused(RuntimeError, SAME, fn, z(3, 5), z(3, 5, dtype=torch.float64), precise=False)
        refused(RuntimeError, FLOATS, fn, z(3, 5, dtype=torch.int32), z(3, 5, dtype=torch.int32), precise=False)
        refused(RuntimeError, FLOATS, fn, z(3, 5, dtype=torch.float16), z(3, 5, dtype=torch.float16), precise=False)
    refused(RuntimeError, SAME, box.box3d_iou_paired, z(3, 7), z(3, 7, dtype=torch.float64), precise=False)
    # `precise` promotes other dtypes to fp64 in the paired fronts; the sparse front keeps its values in the boxes' dtype and refuses
    refused(RuntimeError, SAME, box.box2d_iou_sparse, z(3, 5), z(3, 5, dtype=torch.float64))
    refused(RuntimeError, FLOATS, box.box2d_iou_sparse, z(3, 5, dtype=torch.int32), z(3, 5, dtype=torch.int32))
    refused(RuntimeError, FLOATS, box.box2d_iou_sparse, z(3, 5, dtype=torch.float16), z(3, 5, dtype=torch.float16))


def test_nms_fronts():
    counts = "Numbers of boxes and scores are inconsistent!"
    ids = torch.zeros(3, dtype=torch.int64)
    refused(ValueError, counts, box.box2d_nms, z(3, 5), z(4))
    refused(ValueError, counts, box.box2d_nms_batched, z(3, 5), z(4), ids)
    refused(ValueError, counts, box.box2d_nms_batched, np.zeros((3, 5)), np.zeros(2), np.zeros(3, np.int64))
    for groups in (ids[:2], torch.zeros((3, 1), dtype=torch.int64), np.zeros(4, np.int32)):
        refused(ValueError, "Numbers of boxes and groups are inconsistent!", box.box2d_nms_batched, z(3, 5), z(3), groups)
    refused(TypeError, "groups must be an integer tensor, got torch.float32", box.box2d_nms_batched, z(3, 5), z(3), z(3))
    refused(TypeError, "groups must be an integer tensor, got torch.bool", box.box2d_nms_batched, z(3, 5), z(3), ids.bool())
    refused(TypeError, "groups must be an integer array, got float64", box.box2d_nms_batched, z(3, 5), z(3), np.zeros(3))
    refused(TypeError, "groups must be a torch tensor or a numpy array of integers", box.box2d_nms_batched, z(3, 5), z(3), [0, 0, 0])
    for method in ("linear", "gaussian"):
        refused(ValueError, HARD, box.box2d_nms_batched, z(3, 5), z(3), ids, supression_method=method)
    refused(ValueError, "Unsupported iou type!", box.box2d_nms_batched, z(3, 5), z(3), ids, iou_method="grbox")
    refused(RuntimeError, "boxes and scores must have the same dtype", box.box2d_nms_batched, z(3, 5), z(3).double(), ids, precise=False)
    refused(RuntimeError, FLOATS, box.box2d_nms_batched, z(3, 5).int(), z(3).int(), ids, precise=False)
    for fn, extra in ((box.box2d_nms, ()), (box.box2d_nms_batched, (ids,))):
        with pytest.raises(AttributeError, match="CIRCLE"):
            fn(z(3, 5), z(3), *extra, iou_method="circle")
        with pytest.raises(AttributeError, match="SOFT"):
            fn(z(3, 5), z(3), *extra, supression_method="soft")
        empty = fn(z(0, 5), z(0), *(e[:0] for e in extra))                    # (the empty case answers before any of the names is looked up)
        assert empty.dtype == torch.bool and empty.shape == (0,) and empty.device.type == "cpu"


def test_projection_axis():
    for axis in (3, -1, None):
        refused(ValueError, AXIS, box.box3dp_crop, z(4, 3), z(3, 7), axis)
        refused(ValueError, AXIS, box.box3dr_pdist, z(4, 3), z(3, 7), axis)
        refused(ValueError, AXIS, box.box3dp_crop, z(4096, 3), z(3, 7), axis)     # (the size of the one-launch route: still the axis first)


def test_matcher_refusals():
    for cls in (matcher.ScoreMatcher, matcher.HungarianMatcher, matcher.NearestNeighborMatcher):
        refused(ValueError, ROWS9 % "src_boxes", cls().prepare_boxes, z(3, 8), z(3, 9), 1)
        refused(ValueError, ROWS9 % "dst_boxes", cls().prepare_boxes, np.zeros((3, 9)), np.zeros((3, 8)), 1)
        refused(ValueError, ROWS9 % "src_boxes", cls().prepare_boxes, z(9), z(3, 8), 1)       # (two faults: the sources first)
    for fn in (matcher.hungarian_match, matcher.nearest_neighbor_match):
        refused(ValueError, "distance should be a [n, m] matrix", fn, z(4), [0] * 4, [0] * 4, {0: 1.0})
        refused(ValueError, "distance should be a [n, m] matrix", fn, np.zeros((2, 2, 2)), [0] * 3, [0], {})      # (before the tags)
    shape = "expected a matrix (2-D array) or a batch of matrices (3-D array), got shape %r"
    refused(ValueError, shape % ((4,),), matcher.linear_sum_assignment, np.zeros(4))
    refused(ValueError, shape % ((1, 1, 1, 1),), matcher.linear_sum_assignment, z(1, 1, 1, 1))


def test_the_order_of_the_checks():
    with pytest.raises(AssertionError):                                       # numpy against torch before anything else
        box.box2d_iou_sparse(np.zeros(5), z(3, 4), method="circle", threshold=-1)
    refused(ValueError, NX2, box.box2d_iou, z(5), z(3, 4), method="circle")                   # rank, then width, then the name
    refused(ValueError, F5, box.box2d_iou, z(3, 4), z(3, 5), method="circle")
    refused(ValueError, "threshold should be a finite number >= 0, got -1", box.box2d_iou_sparse, z(5), z(3, 5), threshold=-1)
    refused(ValueError, F5, box.box2d_iou_sparse, z(3, 4), z(3, 5).double(), method="grbox")   # width, name, dtypes
    refused(ValueError, "Unsupported iou type!", box.box2d_iou_sparse, z(3, 5), z(3, 5).double(), method="grbox")
    refused(ValueError, "Unrecognized iou type!", box.box3d_iou_paired, z(3, 6), z(4, 7), method="circle")     # name, width, counts
    refused(ValueError, F7, box.box3d_iou_paired, z(3, 6), z(4, 7))
    refused(ValueError, "threshold should be a finite number >= 0, got nan", box.iou3d_sparse, z(3, 6), z(3, 7), "circle", float("nan"))
    refused(ValueError, "Unrecognized iou type!", box.iou3d_sparse, z(3, 6), z(3, 7), "circle")
    refused(ValueError, F5, box.box2d_iou_paired, z(3, 4), z(4, 5), method="circle")          # width, counts, name, dtypes
    refused(ValueError, "Paired boxes should come in equal numbers: 3 and 4", box.box2d_iou_paired, z(3, 5), z(4, 5), method="circle")
    with pytest.raises(AttributeError):
        box.box2d_iou_paired(z(3, 5), z(3, 5).double(), method="circle", precise=False)
    refused(ValueError, "Numbers of boxes and scores are inconsistent!", box.box2d_nms_batched, z(3, 5), z(4), z(3))      # counts, groups' type,
    refused(TypeError, "groups must be an integer tensor, got torch.float32", box.box2d_nms_batched, z(3, 5), z(3), z(4),  # groups' count, ...
            supression_method="linear")
    ids = torch.zeros(3, dtype=torch.int64)
    refused(ValueError, HARD, box.box2d_nms_batched, z(3, 5), z(3), ids, iou_method="grbox", supression_method="linear")  # ... hard, iou type
    refused(ValueError, "Input boxes should be Nx2 tensors!", box.box2dr_pdist, z(4, 2), z(5), method="box")
    refused(ValueError, F5, box.box2dr_pdist, z(4, 2), z(3, 4), method="box")


def _text(*parts):
    import d3d_amd
    with open(os.path.join(os.path.dirname(d3d_amd.__file__), *parts)) as fh:
        return fh.read()


def test_each_message_and_helper_is_defined_once():
    text = _text("box", "__init__.py")
    for once in (F5, F7):                                                    # the two row-width messages
        assert text.count(once) == 1, once
    text = _text("tracking", "matcher.py")
    assert text.count(".cpu().numpy() if isinstance(") == 1                  # one host conversion
    assert text.count("distance_threshold.get(") == 1                         # one threshold lookup


def test_no_offset_arithmetic_on_a_shipped_buffer():
    """matcher.py takes typed device views from _lib.ship: no `.view(` of a slice anywhere in it"""
    text = _text("tracking", "matcher.py")
    assert re.search(r"\[[^\]\n]*:[^\]\n]*\]\s*(\.to\([^)\n]*\))?\s*\.view\(", text) is None


def test_ship_on_the_host():
    """_lib.ship's layout without a GPU (the copy goes to the CPU device): every view has its input's dtype, shape and values, and
    starts at a multiple of 8 bytes of the one buffer"""
    rng = np.random.default_rng(5)
    pieces = [rng.integers(0, 255, size=5).astype(np.uint8), rng.integers(-9, 9, size=3).astype(np.int64), np.zeros((0,), np.float32),
              rng.normal(size=1).astype(np.float32), rng.integers(0, 255, size=3).astype(np.uint8), rng.integers(-9, 9, size=(5, 1)).astype(np.int32),
              rng.integers(-9, 9, size=1).astype(np.int64), np.zeros((0, 2), np.int64), rng.normal(size=(1, 3)).astype(np.float32)]
    views = _lib.ship(torch.device("cpu"), *pieces)
    assert len(views) == len(pieces)
    base = views[0].data_ptr()
    for a, v in zip(pieces, views):
        assert v.dtype == torch.from_numpy(a).dtype and tuple(v.shape) == a.shape and np.array_equal(v.numpy(), a)
        assert (v.data_ptr() - base) % 8 == 0
    assert _lib.ship(torch.device("cpu")) == ()


def _threshold_models(distance_threshold, tags, classes, counts):
    """the three spellings the one lookup replaced, as they stood"""
    first = np.zeros((tags.size,), np.float32)                                # ReferenceAssociation.__init__
    for tag in np.unique(tags):
        first[tags == tag] = np.float32(float(distance_threshold.get(int(tag), 0.0)))
    second = np.zeros((tags.size,), np.float32)                               # _threshold_of (nearest_neighbor_match)
    for tag in np.unique(tags):
        second[tags == tag] = np.float32(float(distance_threshold.get(int(tag), 0.0)))
    third = np.repeat(np.array([np.float32(float(distance_threshold.get(int(c), 0.0))) for c in classes], np.float32), counts)      # hungarian_match
    return first, second, third


@pytest.mark.parametrize("seed", range(8))
def test_threshold_lookup_against_the_three_spellings(seed):
    rng = np.random.default_rng(seed)
    tags = rng.integers(-2, 9, size=int(rng.integers(0, 40))).astype((np.int64, np.int32)[seed % 2])
    table = {int(t): float(v) for t, v in zip(rng.integers(-2, 12, size=6), rng.normal(size=6) * 10.0 ** rng.integers(-3, 20, size=6))}
    table[int(rng.integers(0, 9))] = 1 / 3                                     # a value fp32 rounds
    if seed % 2:
        table[int(rng.integers(0, 9))] = np.float64(1e-50)                     # and one it flushes
    classes = list(dict.fromkeys(int(t) for t in rng.integers(-2, 12, size=5)))                # distinct, in first-appearance order
    counts = rng.integers(1, 5, size=len(classes))
    first, second, third = _threshold_models(table, tags, classes, counts)
    got = matcher._threshold_of(table, tags)
    assert got.dtype == np.float32 and got.shape == tags.shape
    assert np.array_equal(got.view(np.uint32), first.view(np.uint32)) and np.array_equal(got.view(np.uint32), second.view(np.uint32))
    per_class = np.repeat(matcher._threshold_of(table, np.asarray(classes, np.int64)), counts)  # hungarian_match's use of it
    assert per_class.dtype == np.float32 and np.array_equal(per_class.view(np.uint32), third.view(np.uint32))
    assert matcher._threshold_of({}, tags).tolist() == [0.0] * tags.size
