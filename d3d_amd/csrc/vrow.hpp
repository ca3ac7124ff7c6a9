// vrow.hpp -- what the row kernels of the voxel stack share (vpool.hip, vtpool.hip, vnbr.hip's gather; vconv.hip takes the alignment
// test and the row limit): a row of C channels is served by one lane GROUP, a lane per 16 bytes of it where C and every base
// address allow, per element otherwise.  Here: the packed row, the group's size, the alignment test, the reduction codes, the rule
// by which max / min pick their winner, the step that folds one row into the running result, and the host ladder from
// (dtype, C, alignment, reduction) to the kernel's template arguments.
#pragma once
#include "common.hpp"

namespace {

constexpr int kRowSum = 4;                    // the code for SUM wherever a `reduction` is taken (d3d_voxelize_3d_reduce's)
constexpr int64_t kRowMax = 0x7fffffffll;     // row numbers (order, arg, table entries) are int32

// N elements moved as one load or store
template <typename T, int N> struct alignas(sizeof(T) * N) RowPack { T v[N]; };

// the type the sums are kept in (and the comparisons made in: the conversion is exact and keeps the order, NaN and the zeros)
template <typename T> struct RowAcc { typedef T type; };
template <> struct RowAcc<_Float16> { typedef float type; };
template <> struct RowAcc<__bf16> { typedef float type; };

// The winner of max (min): the first x > best (x < best) in fold order wins; a NaN wins over every number and the FIRST NaN stays;
// -0.0 == +0.0, so the earlier zero stays.
// (two comparisons: !(x <= best) holds for x > best and for an unordered pair, best == best leaves the NaN already there alone)
template <typename A, bool IS_MAX> __device__ __forceinline__ bool row_takes(A best, A x)
{
    return (best == best) & !(IS_MAX ? x <= best : x >= best);
}

// One step of the fold, per channel: MAX / MIN keep the best so far in acc and the id of the row it came from in win (-1: none
// yet, the first row is taken as it is); SUM / MEAN add in A.
template <int RED, typename A, typename T, int VEC>
__device__ __forceinline__ void row_fold(A (&acc)[VEC], int32_t (&win)[VEC], const RowPack<T, VEC> &x, int32_t id)
{
#pragma unroll
    for (int q = 0; q < VEC; q++) {
        if constexpr (RED == D3D_REDUCE_MAX || RED == D3D_REDUCE_MIN) {
            // two selects on one flag, no branch: as `if (take) { acc = x; win = id; }` hipcc 7.2 dropped the update of win for
            // the channels after the first (it kept `win < 0 ? id : win`)
            const A xq = (A)x.v[q];
            const bool take = (win[q] < 0) | row_takes<A, RED == D3D_REDUCE_MAX>(acc[q], xq);
            acc[q] = take ? xq : acc[q];
            win[q] = take ? id : win[q];
        } else acc[q] += (A)x.v[q];
    }
}

// the lane group of a row of c channels in units of vec: the smallest power of two >= ceil(c / vec), at most a wavefront
int row_group_log2(int32_t c, int vec)
{
    const int64_t units = d3d_divup(c, vec);
    int g = 0;
    while (g < 6 && (1ll << g) < units) g++;
    return g;
}

bool row_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

bool row_reduction_ok(int32_t r) { return r == D3D_REDUCE_MEAN || r == D3D_REDUCE_MAX || r == D3D_REDUCE_MIN || r == kRowSum; }

// dtype (one of CODES) -> its types p; VEC = the elements of 16 bytes where c is a multiple of that and `aligned` says that every
// pointer the kernel moves packs through is 16-byte aligned, 1 otherwise; gl = log2 of the lane group of such a row:
// f(p, std::integral_constant<int, VEC>{}, gl) around ONE launch site
template <int... CODES, class F>
int row_dispatch(int dtype, int32_t c, bool aligned, F &&f)
{
    return dispatch_dtype<CODES...>(dtype, [&](auto p) {
        constexpr int W = 16 / (int)sizeof(typename decltype(p)::T);
        const bool vec = aligned && c % W == 0;
        const int gl = row_group_log2(c, vec ? W : 1);
        return dispatch(vec, [&](auto wide) { return f(p, std::integral_constant<int, decltype(wide)::value ? W : 1>{}, gl); });
    });
}
// the same with the reduction: f(p, VEC, std::integral_constant<int, RED>{}, gl)
template <int... CODES, class F>
int row_dispatch(int dtype, int32_t c, bool aligned, int32_t reduction, F &&f)
{
    return row_dispatch<CODES...>(dtype, c, aligned, [&](auto p, auto vec, int gl) {
        return dispatch_int<D3D_REDUCE_MEAN, D3D_REDUCE_MAX, D3D_REDUCE_MIN, kRowSum>(reduction, [&](auto red) { return f(p, vec, red, gl); });
    });
}

}  // namespace
