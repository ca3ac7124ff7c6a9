"""The model of the fused table convolution (csrc/vconv.hip, method="fused" of subm_conv3d / sparse_conv3d / sparse_inverse_conv3d):
the fp64 einsums over a table of voxel_conv_reference / sparse_conv_reference, the rounding to the half types, and the bound a
result computed with fp32 accumulation and one final rounding must keep."""
import numpy as np
import torch

import sparse_conv_reference as sref
import voxel_conv_reference as vref

same_bits = vref.same_bits
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
U = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}        # the unit roundoff of the final rounding (fp32: none beyond E)
EPS_ACC = 2.0 ** -24                                          # the unit roundoff of the fp32 accumulation


def conv(feat, tab, weight, bias=None, mirrored=False):
    """fp64: out[r] = bias + sum_k feat[tab[r, mirrored ? K-1-k : k]] @ weight[k]"""
    return sref.conv(feat, tab[:, ::-1] if mirrored else tab, weight, bias)


def conv_backward(feat, tab, tab_back, weight, grad_out):
    """fp64 -> (grad_features, grad_weight, grad_bias); tab_back: the transposed map (a submanifold table's is its mirrored columns)"""
    return sref.conv_backward(feat, tab, tab_back, weight, grad_out)


def bf16_bits(x32):
    """fp32 -> the uint16 bits of the nearest bfloat16, ties to even (finite values)"""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def round_to(x, kind):
    """fp32 values (given as fp32 or as fp64 that fp32 holds exactly) -> a CPU torch tensor of `kind`, rounded to nearest even"""
    x32 = np.ascontiguousarray(x, np.float32)
    assert np.array_equal(x32.astype(np.float64), np.asarray(x, np.float64)), "not an fp32 value: it would be rounded twice"
    if kind == "f32":
        return torch.from_numpy(x32.copy())
    if kind == "f16":
        return torch.from_numpy(x32.astype(np.float16))
    return torch.from_numpy(bf16_bits(x32).view(np.int16).copy()).view(torch.bfloat16)


def bits(t):
    """a tensor of 2- or 4-byte floats -> its bits as a numpy integer array"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy()


def equal_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def dot_bound(n, magnitude):
    """E: the project's bound of a dot product of length n accumulated in fp32 in any order, (n + 2) 2^-24 sum|a||b|"""
    return (n + 2) * EPS_ACC * magnitude


def result_bound(n, magnitude, exact, kind):
    """|got - exact| of a result accumulated in fp32 and rounded once to `kind`: E (1 + u) + u |exact|"""
    e = dot_bound(n, magnitude)
    return e * (1 + U[kind]) + U[kind] * np.abs(exact)


def magnitudes(feat, tab, tab_back, weight, grad_out, bias=None):
    """sum|a||b| behind every output -> (out, grad_features, grad_weight, grad_bias)"""
    f, w, g = (np.abs(np.asarray(a, np.float64)) for a in (feat, weight, grad_out))
    return (sref.conv(f, tab, w, None if bias is None else np.abs(np.asarray(bias, np.float64))),) + sref.conv_backward(f, tab, tab_back, w, g)
