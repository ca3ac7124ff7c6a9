"""CPU: the paired box operators (box2d_iou_paired, box3d_iou_paired) -- names and bindings, every validation case without a
GPU, the empty case, no silent CPU fallback; and the CPU reference their GPU tests compare against (paired_reference.py) on
known answers."""
import numpy as np
import pytest
import torch

import box_cases as bc
import paired_reference as pr
from d3d_amd import _lib
from d3d_amd import box as dbox
from d3d_amd.box import IouPaired2D, IouPaired3D, box2d_iou_paired, box3d_iou_paired


def test_names_and_bindings():
    for name in ("box2d_iou_paired", "box3d_iou_paired", "IouPaired2D", "IouPaired3D"):
        assert name in dbox.__all__ and hasattr(dbox, name)
    assert issubclass(IouPaired2D, torch.autograd.Function) and issubclass(IouPaired3D, torch.autograd.Function)
    sig = (_lib.ctypes.c_int, [_lib._vp, _lib._vp, _lib._i64, _lib._i32, _lib._i32, _lib._vp, _lib._vp, _lib._vp])
    assert _lib.SIGNATURES["d3d_iou2d_paired"] == sig and _lib.SIGNATURES["d3d_iou3d_paired"] == sig
    lib = _lib.load()                                            # (loading binds every symbol: a missing export raises here)
    # the status codes that need no device: nothing to do, bad size, unknown type
    assert lib.d3d_iou2d_paired(None, None, 0, 2, _lib.F64, None, None, None) == _lib.OK
    assert lib.d3d_iou3d_paired(None, None, 0, 1, _lib.F32_WIDE, None, None, None) == _lib.OK
    assert lib.d3d_iou2d_paired(None, None, -1, 2, _lib.F64, None, None, None) == _lib.ERR_BAD_ARG
    assert lib.d3d_iou2d_paired(None, None, 4, 2, _lib.F64, None, None, None) == _lib.ERR_BAD_ARG       # null pointers, n > 0
    assert lib.d3d_iou3d_paired(None, None, 4, 1, _lib.F32, None, None, None) == _lib.ERR_BAD_ARG
    for iou_type in (0, 3, 5, 7):                                # NA, GBOX, DBOX, out of range
        assert lib.d3d_iou2d_paired(None, None, 0, iou_type, _lib.F64, None, None, None) == _lib.ERR_UNSUPPORTED
    assert lib.d3d_iou2d_paired(None, None, 0, 2, _lib.F64_M32, None, None, None) == _lib.ERR_UNSUPPORTED
    assert lib.d3d_iou3d_paired(None, None, 0, 1, 9, None, None, None) == _lib.ERR_UNSUPPORTED


def test_validation_without_gpu():
    z5, z7 = torch.zeros(3, 5), torch.zeros(3, 7)
    with pytest.raises(AssertionError, match="Input should be both numpy tensor or pytorch tensor!"):
        box2d_iou_paired(np.zeros((3, 5)), z5)
    with pytest.raises(AssertionError, match="Input should be both numpy tensor or pytorch tensor!"):
        box3d_iou_paired(np.zeros((3, 7)), z7)
    for bad in (torch.zeros(5), torch.zeros(3, 5, 1)):           # not 2-D
        with pytest.raises(ValueError):
            box2d_iou_paired(bad, z5)
        with pytest.raises(ValueError):
            box2d_iou_paired(z5, bad)
    with pytest.raises(ValueError):
        box3d_iou_paired(torch.zeros(7), z7)
    with pytest.raises(ValueError, match="5 fields"):
        box2d_iou_paired(torch.zeros(3, 4), z5)
    with pytest.raises(ValueError, match="5 fields"):
        box2d_iou_paired(z5, z7)
    with pytest.raises(ValueError, match="7 fields"):
        box3d_iou_paired(z7, z5)
    with pytest.raises(ValueError, match="equal numbers"):       # new: the pairs must pair up
        box2d_iou_paired(z5, torch.zeros(4, 5))
    with pytest.raises(ValueError, match="equal numbers"):
        box3d_iou_paired(z7, torch.zeros(2, 7))
    with pytest.raises(ValueError, match="equal numbers"):
        box2d_iou_paired(np.zeros((3, 5)), np.zeros((0, 5)))
    # names resolve as in box2d_iou (AttributeError: unknown; ValueError: known to the enum, not offered) and as in iou3d
    with pytest.raises(AttributeError):
        box2d_iou_paired(z5, z5, method="circle")
    for method in ("gbox", "dbox", "na"):
        with pytest.raises(ValueError, match="Unrecognized iou type!"):
            box2d_iou_paired(z5, z5, method=method)
    for method in ("grbox", "circle"):
        with pytest.raises(ValueError, match="Unrecognized iou type!"):
            box3d_iou_paired(z7, z7, method=method)
    with pytest.raises(RuntimeError):                            # not a floating dtype, not promoted
        box2d_iou_paired(torch.zeros(3, 5, dtype=torch.int32), torch.zeros(3, 5, dtype=torch.int32), precise=False)
    with pytest.raises(RuntimeError):                            # two dtypes, not promoted
        box3d_iou_paired(z7, z7.double(), precise=False)


@pytest.mark.parametrize("precise", [True, False])
def test_empty_inputs_give_empty_results_without_gpu(precise):
    for dtype in (torch.float32, torch.float64):
        for method in pr.METHODS_2D:
            out = box2d_iou_paired(torch.zeros(0, 5, dtype=dtype), torch.zeros(0, 5, dtype=dtype), method=method, precise=precise)
            assert torch.is_tensor(out) and out.shape == (0,) and out.dtype == dtype
        out = box3d_iou_paired(torch.zeros(0, 7, dtype=dtype), torch.zeros(0, 7, dtype=dtype), precise=precise)
        assert out.shape == (0,) and out.dtype == dtype
    out = box2d_iou_paired(np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32), precise=precise)
    assert isinstance(out, np.ndarray) and out.shape == (0,) and out.dtype == np.float32
    out = box3d_iou_paired(np.zeros((0, 7)), np.zeros((0, 7)), method="box", precise=precise)
    assert isinstance(out, np.ndarray) and out.shape == (0,) and out.dtype == np.float64


def test_no_silent_cpu_fallback():
    if not torch.cuda.is_available():                            # (with a GPU the calls below simply run: test_gpu_paired.py)
        with pytest.raises(RuntimeError, match="HIP device"):
            box2d_iou_paired(torch.ones(3, 5), torch.ones(3, 5))
        with pytest.raises(RuntimeError, match="HIP device"):
            box3d_iou_paired(np.ones((3, 7)), np.ones((3, 7)), method="box")


def test_reference_reproduces_known_answers():
    b1, b2, c1, c2, w = pr.seeded_pairs()
    assert b1.shape == b2.shape == (pr.N, 5) and c1.shape == c2.shape == (pr.N, 7) and w.shape == (pr.N,)
    for method in pr.METHODS_2D:                                 # identical boxes: 1 under every measure
        assert np.allclose(pr.iou2d(b1, b1, method), 1, atol=1e-12)
    for method in pr.METHODS_3D:
        assert np.allclose(pr.iou3d(c1, c1, method), 1, atol=1e-12)
    v = pr.iou3d(bc.EVAL_DT.astype(np.float64), bc.EVAL_GT.astype(np.float64), "rbox")
    assert v.shape == (1,) and abs(v[0] - bc.EVAL_IOU) < 1e-4    # the evaluator's pair, as test_oracle_box.py
    # the seeded pairs are what the GPU tests were designed on: overlaps under 'box' / 'rbox', signs of the loss values
    counts = {m: int((pr.iou2d(b1, b2, m) != 0).sum()) for m in pr.METHODS_2D}
    assert counts == {"box": 19, "rbox": 14, "grbox": 40, "drbox": 40}
    assert int((pr.iou2d(b1, b2, "grbox") > 0).sum()) == 4 and int((pr.iou2d(b1, b2, "drbox") > 0).sum()) == 4
    import oracle
    for method in pr.METHODS_3D:                                 # the fp64 model against the fp32 oracle of iou3d
        assert np.max(np.abs(pr.iou3d(c1, c2, method) - np.diag(oracle.iou3d(c1, c2, method)))) < 1e-6
    # the matrices' diagonals are the pair values
    assert np.array_equal(pr.iou2d(b1, b2, "rbox"), np.diag(oracle.iou2d_forward(b1, b2, "rbox")))
    assert np.array_equal(pr.iou2d(b1, b2, "grbox"), np.diag(oracle.loss_iou2dr(b1, b2, "grbox")))


def test_reference_gradients_are_settled():
    """central differences at h = 1e-6 (what the GPU tests use) and at h / 4 agree: no seeded pair sits near a kink, so every
    parameter of every pair can be compared"""
    import functools
    b1, b2, c1, c2, w = pr.seeded_pairs()
    for dims, methods in ((2, pr.METHODS_2D), (3, pr.METHODS_3D)):
        for method in methods:
            _, g1, g2 = pr.reference(dims, method)
            fn = functools.partial(pr.iou2d if dims == 2 else pr.iou3d, method=method)
            h1, h2 = pr.central_gradients(fn, *((b1, b2) if dims == 2 else (c1, c2)), w, h=pr.H / 4)
            for a, b in ((g1, h1), (g2, h2)):
                assert np.max(np.abs(a - b)) < 2e-9 * max(1.0, np.abs(a).max()), (dims, method)
            assert np.abs(g1).max() > 0.05 and np.abs(g2).max() > 0.05
