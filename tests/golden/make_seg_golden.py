"""Generate tests/golden/seg_ref_cases.npz by running the REAL reference SegmentationEvaluator (d3d/benchmarks.pyx, the classes
SegmentationStats and SegmentationEvaluator) in this container.  Data only: the reference's text is read at run time, compiled
in a temporary directory and thrown away.

The two classes are taken out of benchmarks.pyx as they are, behind the libc / libcpp cimports they use, with two mechanical
edits that Cython 3 needs:
  * the hinted `insert(hint, pair)` calls (:1015, :1021) do not type-check against Cython 3's const_iterator overloads; they
    become `insert(pair).first` (the same element: the hint is the end iterator of a failed find);
  * NAN / isnan come from libc.math instead of numpy.math.

Cases: seeded frames, semantic and panoptic, several min_points, a background in and outside `classes`.  Every frame has a
point whose gt key is the background key (a gt label outside `classes`): without one, the reference's `counter[bg_key]`
(:1055) inserts into the map it iterates -- undefined behaviour, which the GPU tests check against tests/seg_reference.py
instead.  Also recorded: the reference's single-core CPU time per shape that tools/segeval_profile.py measures.

usage: python tests/golden/make_seg_golden.py [path/to/benchmarks.pyx]"""
import importlib
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

HEADER = """# cython: language_level=3, boundscheck=False, wraparound=False, cdivision=True
# distutils: language = c++
# distutils: include_dirs = %s
cimport cython
from cython.operator cimport dereference as deref
import numpy as np
cimport numpy as np
from enum import Enum
from libc.math cimport NAN, isnan
from libc.stdint cimport uint8_t, uint16_t, uint32_t, uint64_t
from libcpp.vector cimport vector
from libcpp.unordered_map cimport unordered_map
from libcpp.unordered_set cimport unordered_set
from libcpp.pair cimport pair

"""


def build_reference(pyx, tmp):
    src = open(pyx).read()
    start = src.index("@cython.auto_pickle(True)\ncdef class SegmentationStats")
    body = src[start:]
    body, k = re.subn(r"\.insert\((?:gt_iter|pred_iter), (.*)\)$", r".insert(\1).first", body, flags=re.M)
    assert k == 2, k
    with open(os.path.join(tmp, "segref.pyx"), "w") as f:
        f.write(HEADER % np.get_include() + body)
    subprocess.check_call([sys.executable, "-m", "Cython.Build.Cythonize", "-i", "-q", "segref.pyx"], cwd=tmp,
                          stdout=subprocess.DEVNULL)
    sys.path.insert(0, tmp)
    return importlib.import_module("segref")


def case_frame(rng, n, classes, background, outside):
    """instances as runs of points over labels in `classes`, `outside` labels and the background; the prediction relabels and
    re-ids some points, splits some instances; point 0 carries a gt label outside `classes` (see the module docstring)"""
    pool = list(classes) + list(outside) + [background]
    k = int(rng.integers(3, 16))
    lab = rng.choice(pool, k).astype(np.uint8)
    ids = rng.choice(np.array([0, 1, 2, 3, 7, 500, 65535]), k).astype(np.uint16)
    sizes = rng.multinomial(n, rng.dirichlet(np.ones(k)))
    gl, gi = np.repeat(lab, sizes), np.repeat(ids, sizes)
    pl = gl.copy()
    pi = ((gi.astype(np.int64) * 3 + 1) % 65536).astype(np.uint16)
    flip = rng.random(n) < rng.choice([0.0, 0.1, 0.3])
    pl[flip] = rng.choice(pool, int(flip.sum()))
    pi[flip] = rng.integers(0, 4, int(flip.sum()))
    split = rng.random(n) < rng.choice([0.0, 0.2, 0.45])                       # instances split in two ids: IoUs near 0.5
    pi[split] = pi[split] ^ 1
    gl[0] = outside[0]
    return gl, pl, gi, pi


def main():
    pyx = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/d3d/benchmarks.pyx"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ref = build_reference(pyx, tmp)
        rng = np.random.default_rng(2024)
        configs = [  # classes, background, outside-labels, min_points
            ([1, 2, 3, 4, 5], 0, [9, 200], [0, 5, 40]),
            ([0, 1, 2, 3], 0, [6, 255], [0, 12]),                                # background in classes
            ([3, 7, 11, 255], -1, [4, 12], [0, 1, 25]),                          # background -1 -> 255, in classes
            ([10, 20], 5, [0, 30], [0, 3]),
        ]
        c = 0
        for classes, background, outside, mps in configs:
            bgu = background if background >= 0 else 256 + background
            for n in (1, 17, 300, 2500):
                for mp in mps:
                    gl, pl, gi, pi = case_frame(rng, n, classes, bgu, outside)
                    for pano in (False, True):
                        ev = ref.SegmentationEvaluator(classes, background=background, min_points=mp)
                        st = ev.calc_stats(gl, pl, gi, pi) if pano else ev.calc_stats(gl, pl)
                        o = st.as_object()
                        p = "c%d/" % c
                        out[p + "gt_labels"], out[p + "pred_labels"] = gl, pl
                        if pano:
                            out[p + "gt_ids"], out[p + "pred_ids"] = gi, pi
                        out[p + "classes"] = np.array(classes, np.int64)
                        out[p + "params"] = np.array([background, mp], np.int64)
                        counts = np.zeros((6, 256), np.int64)
                        cum = np.zeros((256,), np.float32)
                        for i, name in enumerate(("tp", "fp", "fn", "itp", "ifp", "ifn")):
                            for k, v in o[name].items():
                                counts[i, k] = v
                        for k, v in o["cumiou"].items():
                            cum[k] = v
                        out[p + "counts"], out[p + "cumiou"] = counts, cum
                        c += 1
        # the reference's CPU time on the shapes of tools/segeval_profile.py (best of a few, one core)
        from d3d_amd import synth
        classes = list(range(1, 20))
        shapes = (("frame120k", 120000, 1, 5), ("batch100", 120000, 100, 1), ("frame8m", 8000000, 1, 2))
        for tag, n, frames, reps in shapes:
            frs = [synth.segmentation_frame(n, seed=s) for s in range(min(frames, 10))]
            for pano in (False, True):
                best = np.inf
                for _ in range(reps):
                    ev = ref.SegmentationEvaluator(classes)
                    t0 = time.perf_counter()
                    for f in range(frames):
                        gl, pl, gi, pi = frs[f % len(frs)]
                        ev.calc_stats(gl, pl, gi, pi) if pano else ev.calc_stats(gl, pl)
                    best = min(best, time.perf_counter() - t0)
                out["time/%s_%s" % (tag, "pano" if pano else "sem")] = np.array([best])
                print("%s %s: %.2f ms" % (tag, "pano" if pano else "sem", best * 1e3))
    np.savez_compressed(os.path.join(HERE, "seg_ref_cases.npz"), **out)
    print("wrote", c, "cases")


if __name__ == "__main__":
    main()
