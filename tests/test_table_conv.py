"""CPU: the model and the cases the GPU tests of the fused table convolution lean on, and the refusals of the built library that
need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_conv_cases as scases
import sparse_conv_reference as sref
import table_conv_cases as cases
import table_conv_reference as ref
import voxel_conv_reference as vref


def test_model_equals_dense_conv3d():
    """the einsum over a table against torch's dense conv3d on the densified scene: submanifold (padding 1, read at the active
    sites) and strided (k3 s2 p1, read at the model's output sites)"""
    c, _ = cases.SCENES["v65"]
    r = np.random.default_rng(3)
    cin, cout = 3, 4
    x, w = r.standard_normal((len(c), cin)), r.standard_normal((27, cin, cout))
    shape = tuple(int(a) + 1 for a in c.max(0))
    grid = torch.zeros((1, cin) + shape, dtype=torch.float64)
    grid[0, :, c[:, 0], c[:, 1], c[:, 2]] = torch.from_numpy(x.T.copy())
    wd = torch.from_numpy(w).reshape(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2).contiguous()
    dense = torch.nn.functional.conv3d(grid, wd, padding=1)[0].numpy()
    got = ref.conv(x, vref.table(c, 3), w)
    assert np.allclose(got, dense[:, c[:, 0], c[:, 1], c[:, 2]].T, rtol=0, atol=1e-12)
    oc, _, t_out, _ = sref.build(c, 3, 2, 1, spatial_shape=shape)
    dense = torch.nn.functional.conv3d(grid, wd, stride=2, padding=1)[0].numpy()
    assert np.allclose(ref.conv(x, t_out, w), dense[:, oc[:, 0], oc[:, 1], oc[:, 2]].T, rtol=0, atol=1e-12)


def test_mirrored_and_transposed_maps():
    """the mirrored table is the submanifold table's transposed map, and the backward of the model is the forward through it"""
    fwd, back, src_rows, rows = cases.tables("far_away-k27")
    r = np.random.default_rng(4)
    x, w, g = r.standard_normal((src_rows, 2)), r.standard_normal((27, 2, 3)), r.standard_normal((rows, 3))
    gf, gw, gb = ref.conv_backward(x, fwd, back, w, g)
    assert np.allclose(gf, ref.conv(g, fwd, np.ascontiguousarray(w.transpose(0, 2, 1)), mirrored=True), rtol=0, atol=1e-12)
    want = vref.conv_backward(x, fwd, w, g)
    assert all(np.allclose(a, b, rtol=0, atol=1e-12) for a, b in zip((gf, gw, gb), want))
    fwd, back, _, _ = cases.tables("negative_odd-up-k3s2")
    v, k = np.nonzero(fwd >= 0)
    assert np.array_equal(back[fwd[v, k], k], v) and np.count_nonzero(back >= 0) == len(v)


def test_cases_cover_the_edges():
    names = [c[0] for c in cases.CASES]
    assert len(set(names)) == len(names)
    assert {len(cases.SCENES["line%d" % v][0]) for v in cases.LINE_ROWS} == set(cases.LINE_ROWS)
    assert {cases.tables(c[0])[0].shape[1] for c in cases.CASES} >= {1, 3, 8, 27}
    assert {(c[4], c[5]) for c in cases.CASES} >= set(cases.CHANNELS)
    assert any(cases.tables(c[0])[2] != cases.tables(c[0])[3] for c in cases.CASES)
    fwd = cases.tables("line129-k27-48x16")[0]
    assert np.count_nonzero((fwd >= 0).any(0)) == 3                  # whole columns absent: the skip runs
    assert cases.tables("v4097-k27")[3] > 4096                       # more than one row slab in the weight gradient


@pytest.mark.parametrize("name", [c[0] for c in cases.CASES])
def test_integer_cases_are_exact(name):
    """sum|a||b| of every output and every gradient below 2^24 and below fp16's 65504: every fp32 partial sum is exact"""
    x, w, bias, g = cases.integers(name)
    fwd, back, _, _ = cases.tables(name)
    assert np.abs(x).max() <= 3 and np.abs(w).max() <= 2 and np.abs(g).max() <= 3
    for m in ref.magnitudes(x, fwd, back, w, g, bias):
        assert m.max() < 65504 < 2 ** 24
    out = ref.conv(x, fwd, w, bias)
    assert np.array_equal(out, np.round(out)) and np.array_equal(out.astype(np.float32).astype(np.float64), out)


def test_rounding_helper_matches_torch():
    r = np.random.default_rng(5)
    x = np.concatenate([r.standard_normal(50000) * np.exp2(r.integers(-20, 16, 50000)), np.arange(-4096, 4097) / 8.0,
                        [0.0, -0.0, 1 + 2.0 ** -8, 1 + 2.0 ** -9, 1 + 3 * 2.0 ** -9, 65504.0, 2.0 ** -14]]).astype(np.float32)
    t = torch.from_numpy(x)
    for kind in ("f32", "f16", "bf16"):
        keep = np.abs(x) <= 65504 if kind == "f16" else np.ones(len(x), bool)
        assert ref.equal_bits(ref.round_to(x[keep], kind), t[torch.from_numpy(keep)].to(ref.TORCH[kind]))
    with pytest.raises(AssertionError):
        ref.round_to(np.array([1 + 2.0 ** -30]), "bf16")


def test_bound_shape():
    e = ref.dot_bound(30, np.array([2.0]))
    assert e[0] == 32 * 2.0 ** -24 * 2.0
    assert ref.result_bound(30, np.array([2.0]), np.array([-3.0]), "f32")[0] == e[0]
    assert ref.result_bound(30, np.array([2.0]), np.array([-3.0]), "bf16")[0] == e[0] * (1 + 2.0 ** -8) + 3 * 2.0 ** -8


def test_library_refuses_without_a_gpu():
    """d3d_table_conv answers for an empty launch, fp64 and ineligible channel counts before any HIP call"""
    from d3d_amd import _lib
    lib = _lib.load()
    assert (_lib.F16, _lib.BF16) == (4, 5) and (_lib.F32, _lib.F64, _lib.F64_M32, _lib.F32_WIDE) == (0, 1, 2, 3)
    null = ctypes.c_void_p(0)

    def call(rows, cin, cout, dtype, k=27):
        return lib.d3d_table_conv(null, 10, cin, null, rows, k, 0, null, null, cout, dtype, null, null)
    for dtype in (_lib.F32, _lib.F16, _lib.BF16):
        assert call(0, 16, 32, dtype) == _lib.OK
    assert call(0, 16, 16, _lib.F64) == _lib.ERR_UNSUPPORTED and call(8, 16, 16, _lib.F64) == _lib.ERR_UNSUPPORTED
    for cin, cout in ((5, 16), (16, 5), (272, 16), (16, 24), (8, 16)):
        assert call(8, cin, cout, _lib.F32) == _lib.ERR_UNSUPPORTED and call(0, cin, cout, _lib.BF16) == _lib.ERR_UNSUPPORTED
    assert call(8, 16, 16, _lib.F32, k=344) == _lib.ERR_UNSUPPORTED
    assert call(8, 16, 16, 7) == _lib.ERR_BAD_ARG and call(8, 16, 16, _lib.F32) == _lib.ERR_BAD_ARG       # unknown dtype; no pointers
    assert lib.d3d_table_conv_wgrad(null, 10, 5, null, 8, 27, 0, null, 16, _lib.F32, null, null, 0, null) == _lib.ERR_UNSUPPORTED
    assert lib.d3d_table_conv_wgrad(null, 10, 16, null, 8, 27, 0, null, 16, _lib.F64, null, null, 0, null) == _lib.ERR_UNSUPPORTED
    one = 27 * 16 * 32 * 4
    assert lib.d3d_table_conv_wgrad_workspace_bytes(100, 27, 16, 32) == one
    assert lib.d3d_table_conv_wgrad_workspace_bytes(4097, 27, 16, 32) == 2 * one
    assert lib.d3d_table_conv_wgrad_workspace_bytes(10 ** 6, 27, 16, 32) == 64 * one
    assert lib.d3d_table_conv_wgrad_workspace_bytes(100, 27, 5, 32) == 0


def test_python_refusals_without_a_gpu():
    """the routing table of `method`, on tensors that never reach a device"""
    from d3d_amd.voxel.conv import _conv_dtype, _conv_route
    w = torch.zeros((27, 16, 32))
    x = torch.zeros((4, 16))
    assert _conv_route(x, w, None) == "gather" and _conv_route(x, w, "gather") == "gather" and _conv_route(x, w, "fused") == "fused"
    assert _conv_route(x.double(), w.double(), None) == "gather"
    for t in (torch.float16, torch.bfloat16):
        assert _conv_route(x.to(t), w.to(t), None) == "fused" and _conv_route(x.to(t), w.to(t), "fused") == "fused"
        with pytest.raises(ValueError):
            _conv_route(x.to(t), w.to(t), "gather")
        with pytest.raises(ValueError):
            _conv_route(x.to(t)[:, :5], w.to(t)[:, :5], None)
    for bad in ((x.double(), w.double(), "fused"), (x[:, :5], w[:, :5], "fused"), (x, w[:, :, :24], "fused"), (x, w, "mfma"), (x, w, 1)):
        with pytest.raises(ValueError):
            _conv_route(*bad)
    with pytest.raises(ValueError):
        _conv_dtype(x.to(torch.int32))
