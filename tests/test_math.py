"""d3d_amd.math without a GPU: the numpy model of tests/math_reference.py (what the kernel is specified by) against outputs of
the REAL reference (tests/golden/math_ref_cases.npz, written by tests/golden/make_math_golden.py), those outputs against scipy
and mpmath, the host-side validation of the Python layer and of the C entries, and the reference's own d3d/math/__init__.py
imported against d3d_amd.math.math_impl.  The kernels themselves: tests/test_gpu_math.py."""
import ctypes
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

import math_reference as mr
from golden_io import GOLDEN

Z = np.load(os.path.join(GOLDEN, "math_ref_cases.npz"))
DTYPES = [("f32", np.float32), ("f64", np.float64)]
MODEL = {0: mr.model_i0e, 1: mr.model_i1e}
REF = "/root/reference"


@pytest.mark.parametrize("tag,T", DTYPES)
def test_golden_inputs_are_the_seeded_ones(tag, T):
    x = Z[tag + "/x"]
    assert x.dtype == T and mr.same_bits(x, mr.golden_inputs(T))
    fi = np.finfo(T)
    mag = np.abs(x[np.isfinite(x)])
    assert np.any((mag > 0) & (mag < fi.tiny)) and np.any(mag > 1e30) and np.any(np.isnan(x)) and np.any(np.isinf(x))
    assert np.any(mr.bits(x) == mr.bits(np.array([-0.0], T))[0])
    for v in (8.0, -8.0):                                  # several ulps on each side of the split
        near = x[np.abs(x - T(v)) <= 16 * np.spacing(T(8))]
        assert np.sum(np.abs(near) > 8) >= 8 and np.sum(np.abs(near) < 8) >= 8 and np.any(near == T(v))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("tag,T", DTYPES)
def test_model_equals_every_golden_bit(tag, T, order):
    x, want = Z[tag + "/x"], Z["%s/i%de" % (tag, order)]
    got = MODEL[order](x)
    assert got.dtype == T and mr.same_bits(got, want)
    assert np.array_equal(np.isnan(want), np.isnan(x))     # NaN in, NaN out, nowhere else
    if order == 1:                 # i1e(x) ~ x/2 near 0: the goldens hold subnormal outputs, flushing would be seen
        assert np.any((np.abs(want) > 0) & (np.abs(want) < np.finfo(T).tiny))


def test_reference_fp32_is_not_the_nearest_float():
    """what the issue observed and the contract keeps: i0e(0.0f) of the reference is 1.0000001"""
    assert mr.model_i0e(np.array([0.0], np.float32))[0] == np.nextafter(np.float32(1), np.float32(2))
    assert mr.model_i0e(np.array([0.0]))[0] == 1.0


@pytest.mark.parametrize("order", [0, 1])
def test_golden_fp64_equals_scipy(order):
    from scipy import special
    x, want = Z["f64/x"], Z["f64/i%de" % order]
    assert mr.same_bits((special.i0e, special.i1e)[order](x), want)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("tag,T", DTYPES)
def test_recorded_ulp_figures_are_reproduced(tag, T, order):
    """the reference's largest distance from the mpmath value on the seeded sample, recomputed from the model (= the
    reference, bit for bit) and mpmath here"""
    s = mr.ulp_sample(T)
    assert len(s) == mr.ULP_SAMPLE
    d = mr.ulp_distance(MODEL[order](s), mr.exact(order, s))
    recorded = float(Z["%s/i%de_max_ulp" % (tag, order)][0])
    print(tag, "i%de" % order, "largest distance %.4f ulp, recorded %.4f" % (d.max(), recorded))
    assert d.max() == recorded and 0.5 < recorded < 16


def test_mpmath_model_by_hand():
    import mpmath
    e0, e1 = mr.exact(0, np.array([0.0, 1.0, -1.0, np.inf])), mr.exact(1, np.array([0.0, 1.0, -1.0, -np.inf]))
    assert e0[0] == 1 and e1[0] == 0 and e0[3] == 0 and e1[3] == 0
    with mpmath.workdps(50):                 # the power series at x = 1: I_v(1) = sum (1/4)^k / (k! (k + v)!) / 2^v
        s0 = sum(mpmath.mpf(1) / (4 ** k * mpmath.factorial(k) ** 2) for k in range(40)) * mpmath.exp(-1)
        s1 = sum(mpmath.mpf(1) / (4 ** k * mpmath.factorial(k) * mpmath.factorial(k + 1)) for k in range(40)) / 2 * mpmath.exp(-1)
        assert abs(e0[1] - s0) < mpmath.mpf(10) ** -45 and e0[2] == e0[1] and abs(float(s0) - 0.4657596075936404) < 1e-15
        assert abs(e1[1] - s1) < mpmath.mpf(10) ** -45 and e1[2] == -e1[1] and abs(float(s1) - 0.2079104153497085) < 1e-15
    assert np.array_equal(mr.ulp_distance(np.array([1.0, 0.5], np.float32), [mpmath.mpf(1) + mpmath.mpf(2) ** -23, mpmath.mpf(0.5)]),
                          [1.0, 0.0])


def test_backward_model_by_hand():
    x = np.array([0.0, -0.0, 2.0, -2.0, np.nan])
    g = np.array([3.0, 3.0, 2.0, 2.0, 1.0])
    got = mr.model_backward(x, g)
    assert got[0] == 0 and got[1] == 0 and np.isnan(got[4])
    assert got[2] == 2.0 * (mr.model_i1e(x[2:3])[0] - mr.model_i0e(x[2:3])[0]) and got[3] == -got[2]
    h = 1e-6                                                 # ... and it is the derivative
    num = (mr.model_i0e(np.array([2.0 + h])) - mr.model_i0e(np.array([2.0 - h]))) / (2 * h)
    assert abs(num[0] - got[2] / 2.0) < 1e-9


def test_host_side_validation_without_gpu():
    from d3d_amd import _lib
    from d3d_amd import math as dmath
    from d3d_amd.math import math_impl
    assert dmath.cuda_available is True and math_impl.cuda_available is True
    assert math_impl.i0e is dmath.i0e_cc and math_impl.i1e is dmath.i1e_cc
    assert math_impl.i0e_cuda is dmath.i0e_cuda and math_impl.i1e_cuda is dmath.i1e_cuda
    assert sorted(math_impl.__all__) == ["cuda_available", "i0e", "i0e_cuda", "i1e", "i1e_cuda"]
    for fn in (dmath.i0e_cc, dmath.i1e_cc, dmath.i0e_cuda, dmath.i1e_cuda, dmath.i0e, dmath.i1e):
        for dt in (torch.float16, torch.bfloat16, torch.int64):       # AT_DISPATCH_FLOATING_TYPES: float and double only
            with pytest.raises(RuntimeError, match="not implemented"):
                fn(torch.zeros(4, dtype=dt))
        with pytest.raises(TypeError):
            fn([1.0, 2.0])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):         # no silent CPU fallback
            dmath.i0e(torch.zeros(4))
    lib = _lib.load()
    buf = (ctypes.c_double * 4)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    assert lib.d3d_bessel_e(0, null, 0, _lib.F32, null, null) == _lib.OK                # nothing to do, nothing launched
    assert lib.d3d_i0e_backward(null, null, 0, _lib.F64, null, null) == _lib.OK
    for order in (-1, 2, 7):
        assert lib.d3d_bessel_e(order, p, 4, _lib.F64, p, null) == _lib.ERR_BAD_ARG
    assert lib.d3d_bessel_e(0, p, -1, _lib.F64, p, null) == _lib.ERR_BAD_ARG
    assert lib.d3d_bessel_e(1, null, 4, _lib.F64, p, null) == _lib.ERR_BAD_ARG
    assert lib.d3d_bessel_e(1, p, 4, _lib.F32, null, null) == _lib.ERR_BAD_ARG
    assert lib.d3d_i0e_backward(p, null, 4, _lib.F64, p, null) == _lib.ERR_BAD_ARG
    assert lib.d3d_i0e_backward(p, p, -5, _lib.F32, p, null) == _lib.ERR_BAD_ARG
    odd = ctypes.c_void_p(p.value + 2)                                                   # not on an element boundary
    assert lib.d3d_bessel_e(0, odd, 2, _lib.F32, p, null) == _lib.ERR_BAD_ARG
    for code in (_lib.F64_M32, _lib.F32_WIDE, 9, -1):
        assert lib.d3d_bessel_e(0, p, 4, code, p, null) == _lib.ERR_UNSUPPORTED
        assert lib.d3d_i0e_backward(p, p, 4, code, p, null) == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="unsupported"):
        _lib.check(_lib.ERR_UNSUPPORTED, "i0e")


HOST_HARNESS = """
template <class T, int ORDER> static T one(T x)
{
    const T z = std::fabs(x);
    T v = z <= (T)8 ? series_small<T, ORDER>(z) : series_large<T, ORDER>(z);
    if (ORDER == 1) v = x < (T)0 ? -v : v;
    return v;
}
extern "C" void run_f32(int order, const float *x, long n, float *o)
{
    for (long i = 0; i < n; i++) o[i] = order ? one<float, 1>(x[i]) : one<float, 0>(x[i]);
}
extern "C" void run_f64(int order, const double *x, long n, double *o)
{
    for (long i = 0; i < n; i++) o[i] = order ? one<double, 1>(x[i]) : one<double, 0>(x[i]);
}
"""


def test_kernel_series_text_compiled_for_the_host_gives_the_golden_bits(tmp_path):
    """the tables and the three series functions of bessel.hip, as they stand in the file, compiled by g++ without contraction:
    every rounding the kernel's C++ asks for is where the reference has one.  (What the GPU's code object makes of the same
    text -- its root, its division, its float mode -- is tests/test_gpu_math.py's part.)"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "d3d_amd", "csrc", "bessel.hip")).read()
    body = text[text.index("// [series: begin]"): text.index("// [series: end]")]
    src = tmp_path / "series.cpp"
    src.write_text("#include <cmath>\n#define __device__\n#define __forceinline__ inline\n" + body + HOST_HARNESS)
    so = tmp_path / "series.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    for tag, fn in (("f32", lib.run_f32), ("f64", lib.run_f64)):
        x = np.ascontiguousarray(Z[tag + "/x"])
        for order in (0, 1):
            out = np.empty_like(x)
            fn(order, x.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(len(x)), out.ctypes.data_as(ctypes.c_void_p))
            assert mr.same_bits(out, Z["%s/i%de" % (tag, order)]), (tag, order)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "d3d", "math")), reason="needs the reference checkout")
def test_reference_math_layer_imports_against_math_impl():
    """the reference's own d3d/math/__init__.py, loaded from where it lies with d3d_amd.math.math_impl as the compiled module
    it imports (the way tests/test_dropin_reference.py loads the box and voxel layers); nothing of it is copied"""
    from d3d_amd.math import math_impl
    saved = {k: v for k, v in sys.modules.items() if k == "d3d" or k.startswith("d3d.")}
    for k in saved:
        del sys.modules[k]
    try:
        pkg = types.ModuleType("d3d")
        pkg.__path__ = []
        sys.modules["d3d"] = pkg
        sys.modules["d3d.math.math_impl"] = math_impl
        spec = importlib.util.spec_from_file_location("d3d.math", os.path.join(REF, "d3d", "math", "__init__.py"),
                                                      submodule_search_locations=[os.path.join(REF, "d3d", "math")])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["d3d.math"] = mod
        spec.loader.exec_module(mod)
        assert mod.cuda_available is True
        assert mod.i0e_cc is math_impl.i0e and mod.i1e_cc is math_impl.i1e
        assert mod.i0e_cuda is math_impl.i0e_cuda and mod.i1e_cuda is math_impl.i1e_cuda
        assert issubclass(mod.I0Exp, torch.autograd.Function) and callable(mod.i0e)
        if not torch.cuda.is_available():          # a real call lands in this library (no CPU fallback to fall into)
            with pytest.raises(RuntimeError, match="HIP device"):
                mod.i0e(torch.zeros(3))
    finally:
        for k in [k for k in sys.modules if k == "d3d" or k.startswith("d3d.")]:
            del sys.modules[k]
        sys.modules.update(saved)
