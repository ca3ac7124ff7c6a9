"""d3d_amd.math.math_impl -- stands in for the reference's compiled module `d3d.math.math_impl` (math/math.cpp:4-18): the four
functions and the flag reference d3d/math/__init__.py:3-9 imports, with the compiled signatures (math.h:6-11).  Dropped in as
d3d/math/math_impl.py it runs the reference's own I0Exp on the HIP kernels."""
from . import cuda_available, i0e_cc as i0e, i0e_cuda, i1e_cc as i1e, i1e_cuda

__all__ = ["cuda_available", "i0e", "i1e", "i0e_cuda", "i1e_cuda"]
