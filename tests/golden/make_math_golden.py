"""Generate tests/golden/math_ref_cases.npz by running the REAL reference i0e / i1e (d3d/math/{impl,math}.cpp over
math/bessel.h).  Data only: the reference's sources are compiled where they lie into a temporary directory at generation time,
run and thrown away.

Stored, per dtype (f32, f64): the inputs of math_reference.golden_inputs -- dense +-12, wide +-1e3, log-uniform magnitudes over
the dtype's whole range (subnormals included), 8 ulps on each side of +-8, 0, -0, +-inf, nan and the ends of the range -- and
the reference's i0e and i1e of them; and, per function and dtype, the reference's own largest ulp distance from the mpmath
value on the 20 000 inputs of math_reference.ulp_sample (the sample is seeded, so only the figure is stored).

usage: python tests/golden/make_math_golden.py [path/to/reference]"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_reference(ref, tmp):
    os.environ.setdefault("CXX", "g++")
    os.environ.setdefault("MAX_JOBS", "2")
    from torch.utils.cpp_extension import load
    return load(name="math_impl", sources=[os.path.join(ref, "d3d/math/impl.cpp"), os.path.join(ref, "d3d/math/math.cpp")],
                extra_include_paths=[ref], extra_cflags=["-O2", "-Wno-deprecated-declarations"], build_directory=tmp)


def main():
    import math_reference as mr
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        mod = build_reference(ref, tmp)
        assert mod.cuda_available is False
        fns = {0: mod.i0e, 1: mod.i1e}
        for T, tag in ((np.float32, "f32"), (np.float64, "f64")):
            x = mr.golden_inputs(T)
            out[tag + "/x"] = x
            for order in (0, 1):
                y = fns[order](torch.from_numpy(x)).numpy()
                assert y.dtype == x.dtype and y.shape == x.shape
                out["%s/i%de" % (tag, order)] = y
            s = mr.ulp_sample(T)
            for order in (0, 1):
                y = fns[order](torch.from_numpy(s)).numpy()
                d = mr.ulp_distance(y, mr.exact(order, s))
                out["%s/i%de_max_ulp" % (tag, order)] = np.array([d.max()])
                print("%s i%de: %d golden inputs; largest distance from mpmath on the sample %.4f ulp (at x = %r)"
                      % (tag, order, len(x), d.max(), s[int(np.argmax(d))]))
    path = os.path.join(HERE, "math_ref_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
