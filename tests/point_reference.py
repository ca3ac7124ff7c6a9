"""An fp64 model of d3d.point.aligned_scatter (forward gather and its adjoint), written from the operator's definition
(reference d3d/point/scatter.cpp:22-180) with numpy alone, and the error bounds every aligned_scatter test uses.  No GPU, no
library, no oracle.

    the map is [B, C, D1..Dm], a coordinate row is (b, x1..xm); neighbour j of a row, j = 0 .. 2^m - 1, takes per dimension d
        x > D-1:  cell D-1, factor 1/2          x < 0:  cell 0, factor 1/2
        else bit d of j set:  cell ceil(x), factor 1 + x - ceil(x)      clear:  cell floor(x), factor 1 - x + floor(x)
    LINEAR: w_j = product of the factors, out[i, c] = sum_j map[b, c, cell_j] w_j
    MEAN:   out[i, c] = (sum_j map[b, c, cell_j]) / 2^m
    an integral x (0 and D-1 included) has ceil = floor: the same cell twice with factor 1 each -- the reference's quirk,
    pinned by its recorded outputs; -0.0 is not < 0 and counts as the integer 0.
    backward: image_grad[b, c, cell_j] += grad[i, c] w_j   (MEAN: grad[i, c] / 2^m)

Rounding of the operator in its working precision (unit roundoff u = 2^-24 / 2^-53), which the bounds below count:
  * a factor is evaluated as (1 + x) - ceil or (1 - x) + floor.  The second operation is exact (its result is a multiple of
    the first's last bit and smaller); the FIRST rounds to the spacing of 1 +- x, not of the factor: an absolute error of up to
    u |1 +- x|, which is not small beside a factor close to zero (x = 31 + 2^-19 in fp32: 1 + x rounds to 32, factor 0
    instead of 2^-19).  `ew` below is that budget carried through the product: sum_d u |1 +- x_d| prod_{e != d} (f_e + u |1 +- x_e|),
    an upper bound of prod (f_d + e_d) - prod f_d for |e_d| <= u |1 +- x_d| (telescoping sum).  The factor 1/2 is exact.
  * the product of m factors rounds m - 1 times, the term (map w or grad w) once; MEAN's grad / 2^m is exact.
  * a sum of K terms rounds K - 1 times whatever the order.
"""
import numpy as np

MEAN, LINEAR = 1, 2
U32, U64 = 2.0 ** -24, 2.0 ** -53


def unit(dtype):
    return U64 if np.dtype(dtype) == np.float64 else U32


def neighbours(coord, dims, atype, u=0.0):
    """-> off int64 [N, 2^m] flat cell inside one [D1..Dm] map, w fp64 [N, 2^m] weights (MEAN: 1 / 2^m),
    ew fp64 [N, 2^m] the absolute error a weight evaluated with unit roundoff u may carry (see the module docstring)"""
    c = np.asarray(coord).astype(np.float64)
    n, dim = c.shape[0], c.shape[1] - 1
    assert dim == len(dims) and atype in (MEAN, LINEAR)
    nb = 1 << dim
    off = np.zeros((n, nb), np.int64)
    f = np.ones((n, nb, dim))
    e = np.zeros((n, nb, dim))
    for d in range(dim):
        x, dmax = c[:, d + 1], int(dims[d]) - 1
        hi, lo = x > dmax, x < 0
        inside = ~(hi | lo)
        xi = np.where(inside, x, 0.0)
        flo = np.floor(xi)
        frac = xi - flo                                  # exact: Sterbenz for x >= 1, floor = 0 below
        cei = np.where(frac > 0, flo + 1, flo)
        for j in range(nb):
            up = (j >> d) & 1
            cell = np.where(hi, dmax, np.where(lo, 0, cei if up else flo)).astype(np.int64)
            fac = np.where(frac > 0, frac, 1.0) if up else 1.0 - frac
            off[:, j] = off[:, j] * int(dims[d]) + cell
            f[:, j, d] = np.where(inside, fac, 0.5)
            e[:, j, d] = np.where(inside, u * np.abs(1 + xi if up else 1 - xi), 0.0)
    if atype == MEAN:
        return off, np.full((n, nb), 1.0 / nb), np.zeros((n, nb))
    w = np.prod(f, axis=2)
    fe = f + e
    ew = np.zeros((n, nb))
    for d in range(dim):
        ew += e[:, :, d] * np.prod(np.delete(fe, d, axis=2), axis=2)
    return off, w, ew


def _batch(coord):
    return np.asarray(coord)[:, 0].astype(np.float64).astype(np.int64)       # (int)coord[i][0], scatter.cpp:100


def forward_terms(coord, image, atype, u=0.0, dims=None):
    """-> out, S = sum_j |map w_j|, E = sum_j |map| ew_j, each fp64 [N, C].  `image` is the [B, C, D1..Dm] array, or a
    function (b [N, 1], c [1, C], cell [N, 1]) -> fp64 [N, C] with `dims` = (C, D1..Dm) for a map too large to hold."""
    if callable(image):
        C, dims = int(dims[0]), tuple(int(x) for x in dims[1:])
        cols = np.arange(C, dtype=np.int64)[None, :]
        fetch = lambda b, cell: np.asarray(image(b[:, None], cols, cell[:, None]), np.float64)  # noqa: E731
    else:
        img = np.asarray(image).astype(np.float64)
        C, dims = img.shape[1], img.shape[2:]
        cl = np.ascontiguousarray(np.moveaxis(img.reshape(img.shape[0], C, -1), 1, 2))        # [B, vol, C]
        fetch = lambda b, cell: cl[b, cell]  # noqa: E731
    off, w, ew = neighbours(coord, dims, atype, u)
    b = _batch(coord)
    n = off.shape[0]
    out, S, E = np.zeros((n, C)), np.zeros((n, C)), np.zeros((n, C))
    for j in range(off.shape[1]):
        v = fetch(b, off[:, j])
        out += v * w[:, j, None]
        S += np.abs(v) * w[:, j, None]
        E += np.abs(v) * ew[:, j, None]
    return out, S, E


def forward(coord, image, atype):
    """[N, C] fp64"""
    return forward_terms(coord, image, atype)[0]


def forward_bound(S, dim, u, E=0.0):
    """|got - exact| per element: 3 roundings per factor and one per product step and term (3 m + 1 at most), 2^m - 1 for
    the sum, one for MEAN's division; E = the factors' absolute part (forward_terms with the same u), 0 = left out"""
    return ((1 << dim) + 3 * dim + 2) * u * S + E


def accumulate(coord, grad, atype, dims, cells, slot, u=0.0):
    """the adjoint over `cells` rows: slot int64 [N, 2^m] is the row of each neighbour -> sum, K, A, E as [cells, C]"""
    g = np.asarray(grad).astype(np.float64)
    C = g.shape[1]
    _, w, ew = neighbours(coord, dims, atype, u)
    cols = np.arange(C, dtype=np.int64)[None, :]
    tot, A, E = np.zeros(cells * C), np.zeros(cells * C), np.zeros(cells * C)
    ag = np.abs(g)
    for j in range(slot.shape[1]):
        idx = (slot[:, j, None] * C + cols).ravel()
        tot += np.bincount(idx, weights=(g * w[:, j, None]).ravel(), minlength=cells * C)
        A += np.bincount(idx, weights=(ag * w[:, j, None]).ravel(), minlength=cells * C)
        if u and atype == LINEAR:
            E += np.bincount(idx, weights=(ag * ew[:, j, None]).ravel(), minlength=cells * C)
    K = np.bincount(slot.ravel(), minlength=cells).astype(np.float64)
    return tot.reshape(cells, C), np.repeat(K[:, None], C, 1), A.reshape(cells, C), E.reshape(cells, C)


def backward_terms(coord, grad, atype, image_shape, init=None, u=0.0):
    """-> exact adjoint + init, K contributions per element, A = |init| + sum |contribution|, E = the weights' absolute
    part of the contributions' error; each fp64 of image_shape"""
    B, C, dims = int(image_shape[0]), int(image_shape[1]), tuple(int(x) for x in image_shape[2:])
    vol = int(np.prod(dims, dtype=np.int64))
    off, _, _ = neighbours(coord, dims, atype)
    slot = _batch(coord)[:, None] * vol + off
    if slot.size:
        assert slot.min() >= 0 and slot.max() < B * vol
    parts = accumulate(coord, grad, atype, dims, B * vol, slot, u)
    tot, K, A, E = (np.ascontiguousarray(np.moveaxis(p.reshape(B, vol, C), 1, 2)).reshape(image_shape) for p in parts)
    if init is not None:
        i64 = np.asarray(init).astype(np.float64)
        tot, A = tot + i64, A + np.abs(i64)
    return tot, K, A, E


def backward(coord, grad, atype, image_shape, init=None):
    return backward_terms(coord, grad, atype, image_shape, init)[:3]


def backward_sparse(coord, grad, atype, image_shape, u=0.0):
    """the adjoint into a zero map too large to hold -> flat int64 indices into [B, C, D1..Dm] (sorted by (b, cell), then
    c) and sum, K, A, E at them; every other element of the map is zero"""
    C, dims = int(image_shape[1]), tuple(int(x) for x in image_shape[2:])
    vol = int(np.prod(dims, dtype=np.int64))
    off, _, _ = neighbours(coord, dims, atype)
    key = _batch(coord)[:, None] * vol + off
    uniq, slot = np.unique(key, return_inverse=True)
    tot, K, A, E = accumulate(coord, grad, atype, dims, len(uniq), slot.reshape(key.shape), u)
    flat = ((uniq // vol)[:, None] * C + np.arange(C, dtype=np.int64)[None, :]) * vol + (uniq % vol)[:, None]
    return flat.ravel(), tot.ravel(), K.ravel(), A.ravel(), E.ravel()


def backward_bound(K, A, dim, u, E=0.0):
    """|got - exact| per element: at most 3 m + 1 roundings in one term g w or g / 2^m, K - 1 in a sum of K terms in any
    order (the atomics'), two for the staged sum added to the initial value; E as in forward_bound"""
    return (K + 3 * dim + 4) * u * A + E


# ----------------------------------------------------------------------------------------------------------------------
# The cases both test files walk (tests/test_point.py: model against the C oracle; tests/test_gpu_point.py: kernels against
# both).  A covering subset of atype x dtype x C x map x B x n: every C meets every map once (`sweep`), and along each C and
# along each map the sweep passes through both methods, both dtypes, B = 1, 2, 3, a started image_grad and a zero one;
# the sizes that cross a launch boundary, the long runs and the hot cells are listed by hand below it.
CHANNELS = (1, 5, 7, 8, 9, 31, 32, 33, 64, 100)                 # <= 7: plain route; >= 8: channels-last through the Python layer
MAPS = ((31,), (32,), (33,), (1000,), (1, 33), (5, 7), (32, 32), (40, 50), (1, 1, 1), (3, 4, 5), (8, 8, 8), (7, 11, 13))
K_CAP = 4000                                                    # contributions per element an fp32 case may hold
SWEEP_N = (300, 1, 1000, 37, 0, 2500)


class Case:
    def __init__(self, atype, dtype, C, dims, B, n, init, hot=0, seed=0):
        self.atype, self.dtype, self.C, self.dims, self.B, self.n = atype, np.dtype(dtype), C, tuple(dims), B, n
        self.init, self.hot, self.seed = bool(init), hot, seed
        self.dim, self.u = len(self.dims), unit(dtype)
        self.shape = (B, C) + self.dims

    @property
    def id(self):
        return "%s-%s-C%d-%s-B%d-n%d%s%s" % ("mean" if self.atype == MEAN else "linear", self.dtype.name, self.C,
                                             "x".join(map(str, self.dims)), self.B, self.n, "-init" if self.init else "",
                                             "-hot%d" % self.hot if self.hot else "")

    def make(self):
        """-> coord [n, m+1], image [B, C, D..], grad [n, C] (signed), init [B, C, D..] or None, all of self.dtype"""
        return self.make_points(True)

    def make_points(self, maps=False):
        """make() without the two maps (None in their place) unless `maps`"""
        rng = np.random.default_rng([self.seed, self.C, self.n, self.B, self.atype] + list(self.dims))
        dt, n, m = self.dtype.type, self.n, self.dim
        D = np.array(self.dims, np.float64)
        # uniform over [-1, D + 1): whole part and fraction drawn apart, so that an fp64 coordinate uses its whole mantissa
        xy = (rng.integers(-1, D + 1, (n, m)) + rng.random((n, m))).astype(dt)
        b = rng.integers(0, self.B, n)
        b[:self.B] = np.arange(self.B)[:n]                       # every batch index is used, the last one included
        if n >= 16:
            # edges.  No NaN and nothing at or past 2^31: (int)v is undefined there in the reference as well (scatter.cpp:22-33).
            top = (D - 1).astype(dt)
            rows = [np.zeros(m, dt), -np.zeros(m, dt), rng.integers(0, D, m).astype(dt), top,
                    np.nextafter(top, dt(np.inf)), np.nextafter(top, dt(-np.inf)), np.full(m, -1e9, dt), np.full(m, 1e9, dt)]
            for r, row in enumerate(rows):
                xy[r] = row
            for r in range(8):                                   # and mixed per dimension
                xy[8 + r] = [rows[(r + 3 * d) % 8][d] for d in range(m)]
        if self.hot:                                             # a hot cell: the last rows all clamp to the far corner of the last batch
            xy[n - self.hot:] = (D + rng.random((self.hot, m))).astype(dt)
            xy[n - self.hot::2] = dt(1e9)
            b[n - self.hot:] = self.B - 1
        coord = np.concatenate([b[:, None].astype(dt), xy], 1)
        image = rng.standard_normal(self.shape).astype(dt) if maps else None
        grad = rng.standard_normal((n, self.C)).astype(dt)
        init = rng.standard_normal(self.shape).astype(dt) if self.init and maps else None
        return coord, image, grad, init


def _fit(n, B, dims):
    """a point count that keeps the sweep's contributions per element a factor below K_CAP on the small maps"""
    return min(n, max(1, 100 * B * int(np.prod(dims)) >> len(dims)))


def grid():
    f32, f64 = np.float32, np.float64
    cases = []
    for ci, C in enumerate(CHANNELS):
        for mi, dims in enumerate(MAPS):
            k = ci + mi
            B = 1 + (ci + 2 * mi) % 3
            cases.append(Case((MEAN, LINEAR)[k % 2], (f32, f64)[(k // 2) % 2], C, dims, B, _fit(SWEEP_N[k % 6], B, dims),
                              init=(k // 4) % 2))
    # n C = 255, 256, 257: the last lane of a 256-lane workgroup, a full one, one lane into the next
    for C, n, dims, at, dt in ((1, 255, (33,), LINEAR, f32), (1, 256, (5, 7), MEAN, f32), (1, 257, (3, 4, 5), LINEAR, f64),
                               (5, 51, (32, 32), LINEAR, f32), (8, 32, (7, 11, 13), LINEAR, f32), (32, 8, (31,), MEAN, f64),
                               (64, 4, (8, 8, 8), LINEAR, f32), (8, 32, (1, 33), MEAN, f32)):
        cases.append(Case(at, dt, C, dims, 2, n, init=C != 8, seed=1))
    # long runs (70 001 points on the larger maps; 200 000 on (40, 50) and (7, 11, 13) -- on the latter in fp64 only: a corner
    # cell of 1001 collects 7000 contributions, past the fp32 cap)
    for C, n, dims, at, dt, B, init in ((8, 70001, (1000,), LINEAR, f32, 1, 0), (33, 70001, (40, 50), MEAN, f32, 3, 1),
                                        (5, 70001, (32, 32), LINEAR, f64, 2, 1), (9, 70001, (8, 8, 8), LINEAR, f32, 3, 0),
                                        (64, 70001, (7, 11, 13), MEAN, f64, 2, 1), (64, 200000, (40, 50), LINEAR, f32, 2, 1),
                                        (64, 200000, (7, 11, 13), LINEAR, f64, 2, 0), (7, 200000, (7, 11, 13), MEAN, f64, 3, 1),
                                        (100, 200000, (40, 50), MEAN, f64, 1, 0)):
        cases.append(Case(at, dt, C, dims, B, n, init, seed=2))
    # hot cells: all of `hot` rows clamp to one corner, 2^m contributions each, up to the cap (fp64: far past it)
    for C, dims, at, dt, B, hot, extra in ((9, (5, 7), LINEAR, f32, 2, 3900 // 4, 40), (33, (3, 4, 5), MEAN, f32, 3, 3900 // 8, 40),
                                           (8, (33,), LINEAR, f32, 1, 3900 // 2, 40), (5, (7, 11, 13), LINEAR, f32, 2, 3900 // 8, 300),
                                           (32, (40, 50), LINEAR, f64, 2, 50000, 1000), (64, (32, 32), MEAN, f64, 3, 20000, 100)):
        cases.append(Case(at, dt, C, dims, B, hot + extra, init=C in (9, 32), hot=hot, seed=3))
    return cases
