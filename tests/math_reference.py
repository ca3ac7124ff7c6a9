"""What d3d_amd.math is specified by and judged against, numpy and mpmath only (no GPU, nothing of the product).

model_i0e / model_i1e: the rounding contract of the reference's i0e / i1e (d3d/math/bessel.h as g++ compiles it for x86-64),
one numpy operation per rounding.  z = |x|; z <= 8 takes the series on [0, 8], everything else -- NaN included -- the series on
(8, inf).  Clenshaw over the Chebyshev tables Cephes publishes (i0.c, i1.c), highest degree first.
  fp64: all in fp64.  small: y = z/2 - 2; large: y = 32/z - 2, the series divided by sqrt(z).
  fp32 small: y = float(double(z)/2 - 2); state fp32; a step is t = y*b1 (fp32), t = t - b2 (fp32), b0 = float(double(t) + c_k);
              the result float(0.5 * double(float(b0 - b2))).
  fp32 large: the series in fp64 on y = 32.0/double(z) - 2.0; the result float(series / double(sqrtf(z))).
  i1e: the small series times z (in the dtype); the sign of x.
exact_i0e / exact_i1e: mpmath's besseli(v, |x|) * exp(-|x|) at 50 digits, which shares nothing with the above.
ulp_distance: |got - exact| in units of the dtype's spacing at the exact value."""
import functools

import numpy as np

I0_SMALL = [
    -4.4153416464793395e-18, 3.3307945188222384e-17, -2.431279846547955e-16, 1.715391285555133e-15,
    -1.1685332877993451e-14, 7.676185498604936e-14, -4.856446783111929e-13, 2.95505266312964e-12,
    -1.726826291441556e-11, 9.675809035373237e-11, -5.189795601635263e-10, 2.6598237246823866e-09,
    -1.300025009986248e-08, 6.046995022541919e-08, -2.670793853940612e-07, 1.1173875391201037e-06,
    -4.4167383584587505e-06, 1.6448448070728896e-05, -5.754195010082104e-05, 0.00018850288509584165,
    -0.0005763755745385824, 0.0016394756169413357, -0.004324309995050576, 0.010546460394594998,
    -0.02373741480589947, 0.04930528423967071, -0.09490109704804764, 0.17162090152220877,
    -0.3046826723431984, 0.6767952744094761,
]
I0_LARGE = [
    -7.233180487874754e-18, -4.830504485944182e-18, 4.46562142029676e-17, 3.461222867697461e-17,
    -2.8276239805165836e-16, -3.425485619677219e-16, 1.7725601330565263e-15, 3.8116806693526224e-15,
    -9.554846698828307e-15, -4.150569347287222e-14, 1.54008621752141e-14, 3.8527783827421426e-13,
    7.180124451383666e-13, -1.7941785315068062e-12, -1.3215811840447713e-11, -3.1499165279632416e-11,
    1.1889147107846439e-11, 4.94060238822497e-10, 3.3962320257083865e-09, 2.266668990498178e-08,
    2.0489185894690638e-07, 2.8913705208347567e-06, 6.889758346916825e-05, 0.0033691164782556943,
    0.8044904110141088,
]
I1_SMALL = [
    2.7779141127610464e-18, -2.111421214358166e-17, 1.5536319577362005e-16, -1.1055969477353862e-15,
    7.600684294735408e-15, -5.042185504727912e-14, 3.223793365945575e-13, -1.9839743977649436e-12,
    1.1736186298890901e-11, -6.663489723502027e-11, 3.625590281552117e-10, -1.8872497517228294e-09,
    9.381537386495773e-09, -4.445059128796328e-08, 2.0032947535521353e-07, -8.568720264695455e-07,
    3.4702513081376785e-06, -1.3273163656039436e-05, 4.781565107550054e-05, -0.00016176081582589674,
    0.0005122859561685758, -0.0015135724506312532, 0.004156422944312888, -0.010564084894626197,
    0.024726449030626516, -0.05294598120809499, 0.1026436586898471, -0.17641651835783406,
    0.25258718644363365,
]
I1_LARGE = [
    7.517296310842105e-18, 4.414348323071708e-18, -4.6503053684893586e-17, -3.209525921993424e-17,
    2.96262899764595e-16, 3.3082023109209285e-16, -1.8803547755107825e-15, -3.8144030724370075e-15,
    1.0420276984128802e-14, 4.272440016711951e-14, -2.1015418427726643e-14, -4.0835511110921974e-13,
    -7.198551776245908e-13, 2.0356285441470896e-12, 1.4125807436613782e-11, 3.2526035830154884e-11,
    -1.8974958123505413e-11, -5.589743462196584e-10, -3.835380385964237e-09, -2.6314688468895196e-08,
    -2.512236237870209e-07, -3.882564808877691e-06, -0.00011058893876262371, -0.009761097491361469,
    0.7785762350182801,
]
TABLES = {0: (I0_SMALL, I0_LARGE), 1: (I1_SMALL, I1_LARGE)}
assert [len(t) for t in (I0_SMALL, I0_LARGE, I1_SMALL, I1_LARGE)] == [30, 25, 29, 25]

F32, F64 = np.float32, np.float64


def _clenshaw(y, coeffs):
    """state in y's dtype; the coefficient is added in fp64 and the sum rounded back; returns 0.5 * (b0 - b2) in fp64"""
    S = y.dtype.type
    b0 = np.full(y.shape, S(coeffs[0]), S)
    b1 = np.zeros(y.shape, S)
    b2 = b1
    for c in coeffs[1:]:
        b2, b1 = b1, b0
        t = y * b1
        t = t - b2
        b0 = (t.astype(F64) + F64(c)).astype(S)
    d = b0 - b2
    return F64(0.5) * d.astype(F64)


def _model(order, x):
    x = np.asarray(x)
    T = x.dtype.type
    assert T in (F32, F64)
    small_c, large_c = TABLES[order]
    with np.errstate(all="ignore"):
        z = np.abs(x)
        y = (z.astype(F64) / F64(2.0) - F64(2.0)).astype(T)
        small = _clenshaw(y, small_c).astype(T)
        if order == 1:
            small = small * z
        yl = F64(32.0) / z.astype(F64) - F64(2.0)
        root = np.sqrt(z)                                   # the dtype's own square root (fp32: sqrtf), widened below
        large = (_clenshaw(yl, large_c) / root.astype(F64)).astype(T)
        r = np.where(z <= T(8), small, large)
        if order == 1:
            r = np.where(x < 0, -r, r)
    return r.astype(T)


def model_i0e(x):
    return _model(0, x)


def model_i1e(x):
    return _model(1, x)


def model_backward(x, grad):
    """grad * (i1e(x) - sign(x) * i0e(x)) with the forward bits, three roundings in the dtype; sign(0) = sign(NaN) = 0"""
    x, grad = np.asarray(x), np.asarray(grad)
    T = x.dtype.type
    with np.errstate(all="ignore"):
        sign = (x > 0).astype(T) - (x < 0).astype(T)
        t = sign * model_i0e(x)
        u = model_i1e(x) - t
        return grad * u


# ---------------------------------------------------------------- the independent value

@functools.lru_cache(maxsize=None)
def _exact_one(order, v):
    import mpmath
    with mpmath.workdps(50):
        if v != v:
            return mpmath.nan
        a = mpmath.mpf(abs(v))
        if mpmath.isinf(a):
            return mpmath.mpf(0)
        r = mpmath.besseli(order, a) * mpmath.exp(-a)
        return -r if (order == 1 and v < 0) else r


def exact(order, x):
    """list of mpmath values, one per element of x (an fp32 input is taken at its exact value)"""
    return [_exact_one(order, float(v)) for v in np.asarray(x).ravel()]


def ulp_distance(got, exact_values):
    """per element: |got - exact| / spacing of got's dtype at |exact| (the subnormal spacing below the smallest normal).
    Elements whose exact value is NaN are left out (distance 0)."""
    import mpmath
    got = np.asarray(got)
    T = got.dtype.type
    mant, emin = (24, -126) if T is F32 else (53, -1022)
    out = np.zeros(got.size, F64)
    with mpmath.workdps(50):
        for i, (g, e) in enumerate(zip(got.ravel(), exact_values)):
            if mpmath.isnan(e):
                continue
            ae = abs(e)
            ex = emin if ae == 0 else max(int(mpmath.floor(mpmath.log(ae, 2))), emin)
            spacing = mpmath.ldexp(mpmath.mpf(1), ex - mant + 1)
            out[i] = float(abs(mpmath.mpf(float(g)) - e) / spacing)
    return out


# ---------------------------------------------------------------- inputs

def _tiny_max(T):
    fi = np.finfo(T)
    return float(fi.smallest_subnormal), float(fi.max)


def log_uniform(rng, n, T):
    """magnitudes log-uniform between the smallest subnormal and the largest finite value, random signs"""
    lo, hi = _tiny_max(T)
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    v = (mag * rng.choice([-1.0, 1.0], n)).astype(T)
    return v


def around(value, T, ulps):
    """value and `ulps` neighbours on each side, in T"""
    v = [T(value)]
    for direction in (-np.inf, np.inf):
        c = T(value)
        for _ in range(ulps):
            c = np.nextafter(c, T(direction))
            v.append(c)
    return np.array(sorted(v), T)


def golden_inputs(T):
    """the inputs of tests/golden/math_ref_cases.npz for dtype T (seeded: the generator and the tests agree on them)"""
    rng = np.random.default_rng(1200 + np.dtype(T).itemsize)
    fi = np.finfo(T)
    parts = [rng.uniform(-12, 12, 3000).astype(T), rng.uniform(-1e3, 1e3, 2000).astype(T), log_uniform(rng, 3000, T),
             around(8, T, 8), around(-8, T, 8),
             np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny, -fi.tiny,
                       fi.max, -fi.max, 1.0, -1.0, 1e-30, 1e30], T)]
    if T is F64:
        parts.append(np.array([1e-300, -1e-300, 1e300, -1e300], T))
    return np.concatenate(parts)


ULP_SAMPLE = 20000


def ulp_sample(T):
    """the 20 000 seeded inputs the accuracy figures are taken on: dense +-12, wide +-1e3, log-uniform magnitudes"""
    rng = np.random.default_rng(3400 + np.dtype(T).itemsize)
    return np.concatenate([rng.uniform(-12, 12, 10000).astype(T), rng.uniform(-1e3, 1e3, 6000).astype(T),
                           log_uniform(rng, 4000, T)])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def same_bits(a, b):
    """bit equality, the sign of zero included; NaN matches NaN whatever its payload"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (bits(a) == bits(b))))
