"""d3d_amd.math -- drop-in for d3d.math (reference d3d/math/__init__.py over math/impl.cpp): the exponentially scaled modified
Bessel functions i0e(x) = exp(-|x|) I0(x) and i1e(x) = exp(-|x|) I1(x), elementwise on fp32 / fp64 tensors of any shape, with
the reference's bits (bessel.hip), and the autograd function I0Exp behind i0e."""
import torch

from .. import _lib
from .._rows import FLOAT_CODES, device_of

cuda_available = True


def _prepare(x, name):
    if not torch.is_tensor(x):
        raise TypeError("%s(): argument must be a Tensor, not %s" % (name, type(x).__name__))
    if x.dtype not in FLOAT_CODES:                         # AT_DISPATCH_FLOATING_TYPES (impl.cpp:21, 42)
        raise RuntimeError('"%s" not implemented for \'%s\'' % (name, str(x.dtype).replace("torch.", "")))
    return x.device, device_of(x)


def _bessel_e(order, x):
    """the compiled i0e / i1e (impl.cpp:16-46): a new tensor of x's shape and dtype on x's device"""
    name = "i%de" % order
    odev, dev = _prepare(x, name)
    xs = x.detach().to(dev).contiguous()
    with torch.cuda.device(dev):
        out = torch.empty(xs.shape, dtype=xs.dtype, device=dev)
        _lib.check(_lib.load().d3d_bessel_e(order, _lib.ptr(xs), xs.numel(), FLOAT_CODES[xs.dtype], _lib.ptr(out), _lib.stream_ptr()), name)
    return _lib.to_caller(out, odev, dev)


def i0e_cc(x):
    return _bessel_e(0, x)


def i1e_cc(x):
    return _bessel_e(1, x)


i0e_cuda, i1e_cuda = i0e_cc, i1e_cc


def _i0e_backward(x, grad):
    """grad * (i1e(x) - sign(x) * i0e(x)), the derivative of i0e, in one launch (d3d_i0e_backward)"""
    odev, dev = _prepare(x, "i0e_backward")
    if grad.dtype != x.dtype or grad.shape != x.shape:
        raise RuntimeError("i0e_backward: grad must have x's shape and dtype")
    xs, gs = x.detach().to(dev).contiguous(), grad.detach().to(dev).contiguous()
    with torch.cuda.device(dev):
        out = torch.empty(xs.shape, dtype=xs.dtype, device=dev)
        _lib.check(_lib.load().d3d_i0e_backward(_lib.ptr(xs), _lib.ptr(gs), xs.numel(), FLOAT_CODES[xs.dtype], _lib.ptr(out),
                                                _lib.stream_ptr()), "i0e_backward")
    return _lib.to_caller(out, odev, dev)


class I0Exp(torch.autograd.Function):            # math/__init__.py:11-24
    @staticmethod
    def forward(ctx, x, reference_compat=True):
        ctx.reference_compat = reference_compat
        if not reference_compat:
            ctx.save_for_backward(x)
        return i0e_cc(x)

    @staticmethod
    def backward(ctx, grad):
        if ctx.reference_compat:                 # the reference's (:20-24): the function of the incoming gradient, x unused
            return i1e_cc(grad), None
        x, = ctx.saved_tensors
        return _i0e_backward(x, grad), None


def i0e(x, reference_compat=True):
    """Exponentially scaled modified Bessel function of order 0 with autograd (reference math/__init__.py:26-32).
    reference_compat=True (the default) keeps the reference's backward, which returns i1e(grad) -- i1e applied to the incoming
    gradient instead of grad * d i0e / dx; reference_compat=False gives the derivative,
    grad * (i1e(x) - sign(x) * i0e(x))."""
    return I0Exp.apply(x, reference_compat)


def i1e(x):
    """Exponentially scaled modified Bessel function of order 1 (no autograd, as in the reference)"""
    return i1e_cc(x)


__all__ = ["i0e", "i1e", "I0Exp", "i0e_cc", "i1e_cc", "i0e_cuda", "i1e_cuda", "cuda_available"]
