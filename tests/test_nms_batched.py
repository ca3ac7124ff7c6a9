"""CPU: box2d_nms_batched validates its arguments before it touches the library or a device, and the C entry points of the
grouped NMS are declared in include/d3d_hip.h, bound in d3d_amd/_lib.py and exported by the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("d3d_nms2d_grouped", "d3d_nms2d_grouped_workspace_bytes", "d3d_nms2d_group_max")


def test_grouped_entry_points_are_declared_exported_and_bound():
    from d3d_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3d_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, decl), "include/d3d_hip.h does not declare %s" % name
        assert hasattr(lib, name), "libd3d_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
    assert "the reference has no counterpart" in src[src.index("Hard NMS inside every group"):].lower()
    # pure host functions: the cap is one box per lane of the largest workgroup
    assert _lib.load().d3d_nms2d_group_max() == 1024
    assert _lib.load().d3d_nms2d_grouped_workspace_bytes(100000, 3000) >= 0
    # nothing to do / unsupported: decided before any launch
    f = _lib.load().d3d_nms2d_grouped
    assert f(None, None, None, None, 0, 0, 0, 1, _lib.F32, 0.5, 0.0, None, None, 0, None, 0) == _lib.OK
    assert f(None, None, None, None, 10, 0, 0, 2, _lib.F64, 0.5, 0.0, None, None, 0, None, _lib.NMS_KEEP_MASK) == _lib.OK
    assert f(None, None, None, None, 10, 2, 0, 3, _lib.F32, 0.5, 0.0, None, None, 0, None, 0) == _lib.ERR_UNSUPPORTED
    assert f(None, None, None, None, 10, 2, 0, 1, _lib.F64_M32, 0.5, 0.0, None, None, 0, None, 0) == _lib.ERR_UNSUPPORTED
    assert f(None, None, None, None, 10, 2, 0, 1, _lib.F32, 0.5, 0.0, None, None, 0, None, 0) == _lib.ERR_BAD_ARG     # null pointers
    assert f(None, None, None, None, -1, 2, 0, 1, _lib.F32, 0.5, 0.0, None, None, 0, None, 0) == _lib.ERR_BAD_ARG


def test_operator_is_exported():
    import d3d_amd.box as box
    assert "box2d_nms_batched" in box.__all__ and callable(box.box2d_nms_batched)


@pytest.fixture
def no_device(monkeypatch):
    """the library and the device are out of reach: validation that touches either fails the test"""
    from d3d_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("validation reached the library / the device")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "require_gpu", refuse)


def test_validation_happens_on_the_host(no_device):
    from d3d_amd.box import box2d_nms_batched
    b, s, g = torch.zeros(6, 5), torch.zeros(6), torch.zeros(6, dtype=torch.int64)
    for method in ("linear", "gaussian"):
        with pytest.raises(ValueError, match="hard"):
            box2d_nms_batched(b, s, g, supression_method=method)
    with pytest.raises(ValueError, match="inconsistent"):
        box2d_nms_batched(b, s[:5], g)                               # box2d_nms's own message
    with pytest.raises(ValueError, match="groups"):
        box2d_nms_batched(b, s, g[:5])
    with pytest.raises(ValueError, match="groups"):
        box2d_nms_batched(b, s, torch.zeros(7, dtype=torch.int32))
    for bad in (torch.zeros(6), torch.zeros(6, dtype=torch.float64), torch.zeros(6, dtype=torch.bool), np.zeros(6, np.float32),
                np.zeros(6, bool)):
        with pytest.raises(TypeError):
            box2d_nms_batched(b.numpy() if isinstance(bad, np.ndarray) else b, s.numpy() if isinstance(bad, np.ndarray) else s, bad)
    for method in ("grbox", "drbox", "gbox", "dbox", "na"):
        with pytest.raises(ValueError, match="Unsupported iou type!"):
            box2d_nms_batched(b, s, g, iou_method=method)
    with pytest.raises(AttributeError):                              # unknown names fail like box2d_nms's
        box2d_nms_batched(b, s, g, iou_method="circle")
    with pytest.raises(AssertionError):                              # numpy and torch mixed: _ingress's refusal
        box2d_nms_batched(b.numpy(), s, g)


def test_empty_input_is_box2d_nms_empty_result(no_device):
    from d3d_amd.box import box2d_nms, box2d_nms_batched
    for ids in (torch.zeros(0, dtype=torch.int64), np.zeros(0, np.uint8)):
        got = box2d_nms_batched(torch.zeros(0, 5), torch.zeros(0), ids)
        exp = box2d_nms(torch.zeros(0, 5), torch.zeros(0))
        assert type(got) is type(exp) and got.dtype == exp.dtype and got.shape == exp.shape and got.device == exp.device
    got = box2d_nms_batched(np.zeros((0, 5), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int16))
    assert type(got) is type(box2d_nms(np.zeros((0, 5), np.float32), np.zeros((0, 3), np.float32)))


def test_every_integer_dtype_is_a_group_id(no_device):
    """any integer dtype, any values: equal values stay equal and distinct values distinct on the way to int64"""
    from d3d_amd.box import _group_ids
    for dt in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64):
        hi = np.iinfo(dt).max
        ids = np.array([hi, 0, hi, 1, np.iinfo(dt).min, hi - 1], dt)
        out = _group_ids(ids)
        assert out.dtype == torch.int64 and out.shape == (6,)
        o = out.numpy()
        assert np.array_equal(o[:, None] == o[None, :], ids[:, None] == ids[None, :])
    for dt in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
        out = _group_ids(torch.tensor([3, 0, 3, 1], dtype=dt))
        assert out.dtype == torch.int64 and out.tolist() == [3, 0, 3, 1]
    assert _group_ids(torch.tensor([-5, 1 << 41, -5])).tolist() == [-5, 1 << 41, -5]
    from d3d_amd.box import box2d_nms_batched
    with pytest.raises(AssertionError, match="validation reached"):  # valid arguments: only now is the library asked for
        box2d_nms_batched(torch.zeros(3, 5), torch.zeros(3), torch.zeros(3, dtype=torch.int64))
