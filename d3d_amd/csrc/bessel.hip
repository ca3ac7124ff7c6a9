// bessel.hip -- d3d.math of the reference (d3d/math/impl.cpp:6-46 over math/bessel.h): the exponentially scaled modified Bessel
// functions i0e(x) = exp(-|x|) I0(x) and i1e(x) = exp(-|x|) I1(x), elementwise on fp32 / fp64, and the derivative of i0e for the
// autograd of d3d_amd.math.  Written from the mathematics: Clenshaw's recurrence over the four Chebyshev series Cephes
// publishes (i0.c / i1.c: 30 and 25 coefficients for order 0, 29 and 25 for order 1, the pair split at |x| = 8).
//
// The contract is the reference's bits, so every rounding is placed where its C++ places one (no contraction: the Makefile's
// -ffp-contract=off; fp32 subnormals kept: the code object's default float mode, nothing here changes it):
//   fp64           everything in fp64.  |x| <= 8: y = z/2 - 2; else y = 32/z - 2 and the series is divided by sqrt(z).
//   fp32, |x| <= 8 y = float(double(z)/2 - 2); the recurrence state is fp32, one step = fp32 multiply, fp32 subtract, then the
//                  coefficient added in fp64 and rounded back to fp32 (the tables are fp64: the sum is promoted);
//   fp32, |x| > 8  the whole series in fp64 on y = 32.0/double(z) - 2.0 (an fp64 argument: the recurrence is instantiated for
//                  fp64), divided by the fp32 square root of z, widened, and rounded to fp32 once.
// i1e multiplies the small series by z (in the tensor's dtype) and takes the sign of x.  NaN fails z <= 8 and comes out of the
// large branch as NaN.
//
// Shape of the launch: a lane owns 16 bytes (4 fp32 / 2 fp64) of the OUTPUT's 16-byte grid -- one vector store; the load is
// a 16-byte one as well, aligned when the input sits on the same grid, else left to the hardware's unaligned access.  The
// up to 3 elements in front of the first 16-byte boundary and the up to 3 behind the last whole vector go through the same
// code in a second pass of the grid's first wavefront, one element per lane.  The coefficients are immediates (constexpr
// tables, loops unrolled): no table loads, no scratch.  z <= 8 is decided per wavefront with a ballot: a wavefront whose lanes
// all fall on one side runs that series alone, a mixed one runs both and selects.
#include "common.hpp"

namespace {

constexpr int kBesThreads = 256;

// [series: begin] -- down to [series: end] the text is plain C++ (tests/test_math.py compiles it for the host against the goldens)
constexpr double kI0Small[30] = {
    -4.4153416464793395e-18, 3.3307945188222384e-17, -2.431279846547955e-16, 1.715391285555133e-15,
    -1.1685332877993451e-14, 7.676185498604936e-14, -4.856446783111929e-13, 2.95505266312964e-12,
    -1.726826291441556e-11, 9.675809035373237e-11, -5.189795601635263e-10, 2.6598237246823866e-09,
    -1.300025009986248e-08, 6.046995022541919e-08, -2.670793853940612e-07, 1.1173875391201037e-06,
    -4.4167383584587505e-06, 1.6448448070728896e-05, -5.754195010082104e-05, 0.00018850288509584165,
    -0.0005763755745385824, 0.0016394756169413357, -0.004324309995050576, 0.010546460394594998,
    -0.02373741480589947, 0.04930528423967071, -0.09490109704804764, 0.17162090152220877,
    -0.3046826723431984, 0.6767952744094761};
constexpr double kI0Large[25] = {
    -7.233180487874754e-18, -4.830504485944182e-18, 4.46562142029676e-17, 3.461222867697461e-17,
    -2.8276239805165836e-16, -3.425485619677219e-16, 1.7725601330565263e-15, 3.8116806693526224e-15,
    -9.554846698828307e-15, -4.150569347287222e-14, 1.54008621752141e-14, 3.8527783827421426e-13,
    7.180124451383666e-13, -1.7941785315068062e-12, -1.3215811840447713e-11, -3.1499165279632416e-11,
    1.1889147107846439e-11, 4.94060238822497e-10, 3.3962320257083865e-09, 2.266668990498178e-08,
    2.0489185894690638e-07, 2.8913705208347567e-06, 6.889758346916825e-05, 0.0033691164782556943,
    0.8044904110141088};
constexpr double kI1Small[29] = {
    2.7779141127610464e-18, -2.111421214358166e-17, 1.5536319577362005e-16, -1.1055969477353862e-15,
    7.600684294735408e-15, -5.042185504727912e-14, 3.223793365945575e-13, -1.9839743977649436e-12,
    1.1736186298890901e-11, -6.663489723502027e-11, 3.625590281552117e-10, -1.8872497517228294e-09,
    9.381537386495773e-09, -4.445059128796328e-08, 2.0032947535521353e-07, -8.568720264695455e-07,
    3.4702513081376785e-06, -1.3273163656039436e-05, 4.781565107550054e-05, -0.00016176081582589674,
    0.0005122859561685758, -0.0015135724506312532, 0.004156422944312888, -0.010564084894626197,
    0.024726449030626516, -0.05294598120809499, 0.1026436586898471, -0.17641651835783406,
    0.25258718644363365};
constexpr double kI1Large[25] = {
    7.517296310842105e-18, 4.414348323071708e-18, -4.6503053684893586e-17, -3.209525921993424e-17,
    2.96262899764595e-16, 3.3082023109209285e-16, -1.8803547755107825e-15, -3.8144030724370075e-15,
    1.0420276984128802e-14, 4.272440016711951e-14, -2.1015418427726643e-14, -4.0835511110921974e-13,
    -7.198551776245908e-13, 2.0356285441470896e-12, 1.4125807436613782e-11, 3.2526035830154884e-11,
    -1.8974958123505413e-11, -5.589743462196584e-10, -3.835380385964237e-09, -2.6314688468895196e-08,
    -2.512236237870209e-07, -3.882564808877691e-06, -0.00011058893876262371, -0.009761097491361469,
    0.7785762350182801};

template <int ORDER> struct Series;
template <> struct Series<0> {
    static constexpr int kSmall = 30, kLarge = 25;
    static constexpr double small(int k) { return kI0Small[k]; }
    static constexpr double large(int k) { return kI0Large[k]; }
};
template <> struct Series<1> {
    static constexpr int kSmall = 29, kLarge = 25;
    static constexpr double small(int k) { return kI1Small[k]; }
    static constexpr double large(int k) { return kI1Large[k]; }
};

// Clenshaw over c[0 .. N-1] (highest degree first) with the state in S: one step is S multiply, S subtract, and the fp64
// coefficient added in fp64 (S = float: widened for it, rounded back on assignment).  Returns 0.5 * (b0 - b2) in fp64 -- exact
// for S = double, and for S = float the S-rounded difference halved in fp64, which the caller rounds to fp32.
template <class S, int ORDER, bool SMALL>
__device__ __forceinline__ double clenshaw(S y)
{
    constexpr int N = SMALL ? Series<ORDER>::kSmall : Series<ORDER>::kLarge;
    S b0 = (S)(SMALL ? Series<ORDER>::small(0) : Series<ORDER>::large(0)), b1 = (S)0, b2 = (S)0;
#pragma unroll
    for (int k = 1; k < N; k++) {
        b2 = b1;
        b1 = b0;
        S t = y * b1;
        t = t - b2;
        b0 = (S)((double)t + (SMALL ? Series<ORDER>::small(k) : Series<ORDER>::large(k)));
    }
    const S d = b0 - b2;
    return 0.5 * (double)d;
}

template <class T, int ORDER>
__device__ __forceinline__ T series_small(T z)
{
    const T y = (T)((double)z / 2.0 - 2.0);
    const T s = (T)clenshaw<T, ORDER, true>(y);
    return ORDER == 1 ? s * z : s;
}

template <class T, int ORDER>
__device__ __forceinline__ T series_large(T z)
{
    const double y = 32.0 / (double)z - 2.0;
    const double s = clenshaw<double, ORDER, false>(y);
    // sqrtf / sqrt, not __fsqrt_rn: in this toolchain sqrtf compiles to v_sqrt_f32 plus the two-fma correction that makes it
    // the correctly rounded root, and the intrinsic to the bare 1-ulp v_sqrt_f32 (read off the ISA)
    T root;
    if constexpr (sizeof(T) == 4) root = sqrtf(z);
    else root = sqrt(z);
    return (T)(s / (double)root);
}

// [series: end]

// V values of a lane at once (V independent recurrences in flight).  ORDER 0 / 1: that function; ORDER 2: both, for the
// backward (r0 = i0e, r1 = i1e).  The side of 8 is decided for the wavefront: `any_small` / `any_large` are wave-uniform.
template <class T, int ORDER, int V>
__device__ __forceinline__ void bessel_values(const T (&x)[V], T (&r0)[V], T (&r1)[V])
{
    T z[V];
    bool sm[V], lane_small = false, lane_large = false;
#pragma unroll
    for (int k = 0; k < V; k++) {
        z[k] = fabs(x[k]);       // (order 0 of the reference negates x < 0 and so keeps -0: z/2 - 2 is -2 either way)
        sm[k] = z[k] <= (T)8;
        lane_small |= sm[k];
        lane_large |= !sm[k];
    }
    const bool any_small = __ballot(lane_small) != 0ull, any_large = __ballot(lane_large) != 0ull;
    T a0[V], a1[V], l0[V], l1[V];
#pragma unroll
    for (int k = 0; k < V; k++) a0[k] = a1[k] = l0[k] = l1[k] = (T)0;
    if (any_small) {
#pragma unroll
        for (int k = 0; k < V; k++) {
            if (ORDER != 1) a0[k] = series_small<T, 0>(z[k]);
            if (ORDER != 0) a1[k] = series_small<T, 1>(z[k]);
        }
    }
    if (any_large) {
#pragma unroll
        for (int k = 0; k < V; k++) {
            if (ORDER != 1) l0[k] = series_large<T, 0>(z[k]);
            if (ORDER != 0) l1[k] = series_large<T, 1>(z[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < V; k++) {
        r0[k] = sm[k] ? a0[k] : l0[k];
        const T v = sm[k] ? a1[k] : l1[k];
        r1[k] = x[k] < (T)0 ? -v : v;
    }
}

// 16 bytes of T without the alignment: what a lane loads when the input is not on the output's 16-byte grid
template <class T> struct __attribute__((packed, aligned(sizeof(T)))) Loose { T v[16 / sizeof(T)]; };
template <class T> struct __attribute__((aligned(16))) Tight { T v[16 / sizeof(T)]; };

// the elements of [0, n): `head` single ones, `nvec` vectors of V from the output's first 16-byte boundary on, `tail` single ones
struct Split { int64_t nvec; int head, tail; };

template <class T>
static inline Split split_of(const void *out, int64_t n)
{
    constexpr int V = 16 / sizeof(T);
    Split s;
    const int64_t to_boundary = (int64_t)(((16 - ((uintptr_t)out & 15)) & 15) / sizeof(T));
    s.head = (int)(to_boundary < n ? to_boundary : n);
    s.nvec = (n - s.head) / V;
    s.tail = (int)(n - s.head - s.nvec * V);
    return s;
}

// BACKWARD: out = grad * (i1e(x) - sign(x) * i0e(x)), sign(0) = sign(NaN) = 0; the multiply, the subtract and the multiply in T
template <class T, int ORDER, bool BACKWARD, int V>
__device__ __forceinline__ void finish(const T (&x)[V], const T (&g)[V], T (&out)[V])
{
    T r0[V], r1[V];
    bessel_values<T, BACKWARD ? 2 : ORDER, V>(x, r0, r1);
#pragma unroll
    for (int k = 0; k < V; k++) {
        if (BACKWARD) {
            const T sign = (T)((T)0 < x[k]) - (T)(x[k] < (T)0);
            const T t = sign * r0[k];
            const T u = r1[k] - t;
            out[k] = g[k] * u;
        } else {
            out[k] = ORDER == 0 ? r0[k] : r1[k];
        }
    }
}

template <class T, int ORDER, bool BACKWARD>
__global__ __launch_bounds__(kBesThreads) void k_bessel(const T *x, const T *grad, T *out, Split sp)   // (out may be x or grad)
{
    constexpr int V = 16 / sizeof(T);
    const int64_t stride = (int64_t)gridDim.x * kBesThreads;
    const T *xv = x + sp.head, *gv = grad + sp.head;
    T *ov = out + sp.head;
    for (int64_t i = (int64_t)blockIdx.x * kBesThreads + threadIdx.x; i < sp.nvec; i += stride) {
        const Loose<T> la = *reinterpret_cast<const Loose<T> *>(xv + i * V);
        Loose<T> lb = la;
        if (BACKWARD) lb = *reinterpret_cast<const Loose<T> *>(gv + i * V);
        T a[V], b[V], r[V];
#pragma unroll
        for (int k = 0; k < V; k++) { a[k] = la.v[k]; b[k] = lb.v[k]; }
        finish<T, ORDER, BACKWARD, V>(a, b, r);
        Tight<T> t;
#pragma unroll
        for (int k = 0; k < V; k++) t.v[k] = r[k];
        *reinterpret_cast<Tight<T> *>(ov + i * V) = t;
    }
    // the single elements: the grid's first wavefront, lane j < head -> element j, the next `tail` lanes -> the elements behind
    // the vectors (head + tail <= 2 (V - 1) <= 6 lanes)
    if (blockIdx.x == 0 && threadIdx.x < kWave && (int)threadIdx.x < sp.head + sp.tail) {
        const int j = (int)threadIdx.x;
        const int64_t e = j < sp.head ? (int64_t)j : (int64_t)sp.head + sp.nvec * V + (j - sp.head);
        T a[1] = {x[e]}, b[1] = {a[0]}, r[1];
        if (BACKWARD) b[0] = grad[e];
        finish<T, ORDER, BACKWARD, 1>(a, b, r);
        out[e] = r[0];
    }
}

template <int ORDER, bool BACKWARD>
static int launch(const void *x, const void *grad, int64_t n, int32_t dtype, void *out, hipStream_t st)
{
    if (n < 0) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64) return D3D_ERR_UNSUPPORTED;
    if (n == 0) return D3D_OK;
    if (!x || !out || (BACKWARD && !grad)) return D3D_ERR_BAD_ARG;
    const uintptr_t esize = dtype == D3D_F32 ? 4 : 8;
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)grad) & (esize - 1)) return D3D_ERR_BAD_ARG;      // element alignment
    return dispatch_dtype<D3D_F32, D3D_F64>(dtype, [&](auto p) -> int {
        typedef typename decltype(p)::T T;
        const Split sp = split_of<T>(out, n);
        int64_t blocks = d3d_divup(sp.nvec, kBesThreads);
        if (blocks < 1) blocks = 1;                              // (the single elements alone)
        if (blocks > 0x7fffffffll) blocks = 0x7fffffffll;        // (the kernel strides over the rest)
        const char *name = BACKWARD ? "k_i0e_backward" : ORDER == 0 ? "k_i0e" : "k_i1e";
        D3D_LAUNCH(name, (k_bessel<T, ORDER, BACKWARD>), dim3((unsigned)blocks), dim3(kBesThreads), 0, st, (const T *)x, (const T *)grad,
                   (T *)out, sp);
        return D3D_OK;
    });
}

}  // namespace

// i0e / i1e[_cuda] of the reference (d3d/math/impl.cpp:16-46, math/bessel.h): out[i] = i{order}e(x[i]), i < n.
extern "C" int d3d_bessel_e(int32_t order, const void *x, int64_t n, int32_t dtype, void *out, void *stream)
{
    if (order != 0 && order != 1) return D3D_ERR_BAD_ARG;
    return order == 0 ? launch<0, false>(x, nullptr, n, dtype, out, (hipStream_t)stream)
                      : launch<1, false>(x, nullptr, n, dtype, out, (hipStream_t)stream);
}

// the derivative the reference's I0Exp.backward (d3d/math/__init__.py:19-24) does not compute:
// grad_x[i] = grad[i] * (i1e(x[i]) - sign(x[i]) * i0e(x[i]))
extern "C" int d3d_i0e_backward(const void *x, const void *grad, int64_t n, int32_t dtype, void *grad_x, void *stream)
{
    return launch<0, true>(x, grad, n, dtype, grad_x, (hipStream_t)stream);
}
