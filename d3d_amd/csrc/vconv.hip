// vconv.hip -- the table form of a sparse convolution on the matrix cores of MI355X (gfx950): out[r] = sum_k feat[table[r,k]] @ W[k]
// without the gathered [rows, K * C] buffer, in fp32, fp16 and bf16.  An extension: the reference stops at the voxelizer.
//
//   d3d_table_conv        feat[V,Cin], table[R,K], W[K,Cin,Cout] (+ bias) -> out[R,Cout]: the forward of subm_conv3d, sparse_conv3d and
//                         sparse_inverse_conv3d, and their grad_features (the backward table, W transposed to [K,Cout,Cin] by the host)
//   d3d_table_conv_wgrad  feat[V,Cin], table[R,K], grad_out[R,Cout] -> grad_W[K,Cin,Cout] = sum_r feat[table[r,k]]^T (x) grad_out[r]
//
// k_table_conv: one launch.  A workgroup of 4 wavefronts owns 128 output rows and all of Cout, a wavefront 32 of the rows: 2 x Cout/16
//   accumulator blocks of 16 x 16 in fp32 registers.  For every column kk, in ascending order: the 128 entries of the column (fetched
//   one column ahead) go to LDS and every wavefront ballots them; a column no row of the tile has is skipped.  Otherwise, per stage of
//   128 bytes of input channels (32 fp32 / 64 half): the present rows are gathered into LDS (zeros for the absent ones and for the
//   channels that pad Cin to the MFMA's depth), W[kk]'s rows of the stage go to LDS beside them, and every wavefront multiplies its
//   rows.  A 16-row block without an entry skips its MFMAs: adding a zero product is exact, so a row's bits are a function of its own
//   table row, the rows it points at, W and the bias -- not of its position, of the other rows or of the run.
//     fp32: v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fma chain); A[i][k] and B[k][j] one float per lane, W row-major in LDS
//     half: v_mfma_f32_16x16x32_{f16,bf16}; lane l holds A[l & 15][8 (l >> 4) + j] and B[8 (l >> 4) + j][l & 15], j = 0..7: 16
//           contiguous bytes of an LDS row for A, and of a TRANSPOSED W for B -- a lane fetches an 8 x 8 block of W[kk] as 8 rows of
//           16 bytes, transposes it in registers and stores 8 rows of 16 bytes ([Cout][64 + pad], the 16-byte units of a row XOR-ed
//           with the row's block number: the stores of 8 neighbouring lanes land on 8 different bank groups)
//   Bias is added in fp32, the sum rounded once (RNE) to the output type.
// k_table_conv_wgrad: the reduction runs over the rows, so the present (row, entry) pairs of a column are compacted, in row order,
//   before they feed the MFMA.  Workgroups over (kk, row slab, 64 x 64 block of [Cin, Cout]); the slab count is a function of the
//   sizes alone.  Per 256 rows: ballot + prefix -> the pair list in LDS; per batch of the list (128 pairs half / 64 fp32, zero rows
//   up to the MFMA's depth) the feat rows and grad_out rows go to LDS (half: transposed by the same 8 x 8 register transposition,
//   rows = channels), and wavefront w multiplies channels 16 w .. 16 w + 15 by the 64 output channels.  fp32 partials [S,K,Cin,Cout]
//   go to the workspace; k_table_conv_fold adds the slabs in ascending order and rounds once.  No float atomics; every dependency
//   is a kernel boundary; the order of every sum is fixed by the table and the sizes.
#include <algorithm>
#include "vrow.hpp"                         // (the alignment test and the row limit)

namespace {

constexpr int kTcThreads = 256;
constexpr int kTcTile = 128;                 // output rows of a workgroup (32 per wavefront)
constexpr int kTcStageBytes = 128;           // input channels of a stage, in bytes
constexpr int kTcRowStride = 144;            // an LDS row of a stage: 128 bytes + 16 (rows 36 banks apart)
constexpr int kWgPairsHalf = 128, kWgPairsF32 = 64;      // pairs of a wgrad batch
constexpr int kWgStrideHalf = 272;           // bytes: 128 pairs x 2 + 16
constexpr int kWgStrideF32 = 80;             // floats: 64 channels + 16 (rows 16 banks apart)
constexpr int kWgMaxSlabs = 64;
constexpr int64_t kWgSlabRows = 4096;
constexpr size_t kWgPartialBytes = (size_t)1 << 28;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 tc_mfma(uint4 a, uint4 b, f32x4 c, _Float16)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 tc_mfma(uint4 a, uint4 b, f32x4 c, __bf16)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 tc_mfma(uint4, uint4, f32x4 c, float) { return c; }       // (never called: fp32 has its own loop)
__device__ __forceinline__ f32x4 tc_mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// 16 bytes from p: one load where the buffers are 16-byte aligned, element by element otherwise
template <typename T>
__device__ __forceinline__ uint4 tc_load16(const T *p, bool aligned)
{
    if (aligned) return *(const uint4 *)p;
    union { uint4 v; T e[16 / sizeof(T)]; } u;
#pragma unroll
    for (int i = 0; i < (int)(16 / sizeof(T)); i++) u.e[i] = p[i];
    return u.v;
}

__device__ __forceinline__ uint32_t tc_word(const uint4 &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// in[i] = 8 values of 16 bits (row i of an 8 x 8 block) -> column j of the block: in[0 .. 7]'s value j, as 16 bytes
__device__ __forceinline__ uint4 tc_column(const uint4 (&in)[8], int j)
{
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t a = tc_word(in[2 * d], j >> 1), b = tc_word(in[2 * d + 1], j >> 1);
        o[d] = (j & 1) ? ((a >> 16) | (b & 0xffff0000u)) : ((a & 0xffffu) | (b << 16));
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// the bytes of W[kk]'s stage in LDS: half [cout][kTcRowStride]; fp32 [32][stride floats], the rows 16 banks apart
__host__ __device__ inline int tc_wstride_f32(int cout) { return cout + (cout % 32 == 0 ? 16 : 0); }
template <typename T> size_t tc_lds_bytes(int cout)
{
    const size_t b = sizeof(T) == 4 ? (size_t)32 * tc_wstride_f32(cout) * 4 : (size_t)cout * kTcRowStride;
    return (size_t)kTcTile * kTcRowStride + b + 2 * kTcTile * sizeof(int32_t);
}

template <typename T, int NT>
__global__ __launch_bounds__(kTcThreads) void k_table_conv(const T *__restrict__ feat, int32_t cin, const int32_t *__restrict__ table,
                                                           int64_t rows, int32_t K, int32_t mirrored, const T *__restrict__ weight,
                                                           const T *__restrict__ bias, int32_t cout, int32_t aligned, T *__restrict__ out)
{
    extern __shared__ uint4 tc_smem[];
    constexpr bool kF32 = sizeof(T) == 4;
    constexpr int EPU = 16 / (int)sizeof(T), KC = kTcStageBytes / (int)sizeof(T);
    char *sA = (char *)tc_smem;                                          // [128][kTcRowStride]: the gathered rows of the stage
    char *sB = sA + kTcTile * kTcRowStride;                              // W[kk]'s rows of the stage
    const int wstride = tc_wstride_f32(cout);
    int32_t *sE = (int32_t *)(sB + (kF32 ? 32 * wstride * 4 : cout * kTcRowStride));      // [2][128]: the column's entries

    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6, lr = lane & 15, g = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * kTcTile;
    const bool al = aligned != 0;
    f32x4 acc[2][NT];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < NT; n++) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const bool owner = t < kTcTile && r0 + t < rows;                     // the thread that fetches row t's entries
    const int32_t *trow = table + (owner ? (r0 + t) * (int64_t)K : 0);
    int32_t e_next = owner ? trow[mirrored ? K - 1 : 0] : -1;

    for (int kk = 0; kk < K; kk++) {
        int32_t *se = sE + (kk & 1) * kTcTile;
        if (t < kTcTile) se[t] = e_next;
        if (kk + 1 < K && owner) e_next = trow[mirrored ? K - 2 - kk : kk + 1];
        __syncthreads();                                                  // the entries are in; the last stage's reads are over
        const unsigned long long m0 = __ballot(se[lane] >= 0), m1 = __ballot(se[64 + lane] >= 0);
        if (!(m0 | m1)) continue;                                         // (the same verdict in every wavefront)
        const uint32_t mine = (uint32_t)((w < 2 ? m0 : m1) >> ((w & 1) * 32));
        const bool has[2] = {(mine & 0xffffu) != 0, (mine >> 16) != 0};
        const T *wk = weight + (int64_t)kk * cin * cout;
        for (int kc0 = 0; kc0 < cin; kc0 += KC) {
            if (kc0) __syncthreads();
            const int kn = min(KC, cin - kc0);                            // channels of this stage
            const int units = kF32 ? kn / 4 : (kn + 31) / 32 * 4;         // 16-byte units of a row the MFMAs read
            for (int u = t; u < kTcTile * 8; u += kTcThreads) {
                const int row = u >> 3, c = u & 7;
                if (c >= units) continue;
                const int32_t e = se[row];
                uint4 v = make_uint4(0, 0, 0, 0);
                if (e >= 0 && c * EPU < kn) v = tc_load16(feat + (int64_t)e * cin + kc0 + c * EPU, al);
                *(uint4 *)(sA + row * kTcRowStride + c * 16) = v;
            }
            if (kF32) {
                const int per = cout / 4;
                for (int u = t; u < kn * per; u += kTcThreads) {
                    const int k = u / per, c = u - k * per;
                    *(uint4 *)(sB + ((size_t)k * wstride + c * 4) * 4) = tc_load16(wk + (int64_t)(kc0 + k) * cout + c * 4, al);
                }
            } else {
                const int per = cout / 8;
                for (int b = t; b < units * per; b += kTcThreads) {
                    const int kb = b / per, nb = b - kb * per;
                    uint4 in[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const int k = kb * 8 + i;
                        in[i] = k < kn ? tc_load16(wk + (int64_t)(kc0 + k) * cout + nb * 8, al) : make_uint4(0, 0, 0, 0);
                    }
#pragma unroll
                    for (int j = 0; j < 8; j++) *(uint4 *)(sB + (nb * 8 + j) * kTcRowStride + ((kb ^ (nb & 7)) * 16)) = tc_column(in, j);
                }
            }
            __syncthreads();
            if (!has[0] && !has[1]) continue;
            const int arow = (32 * w + lr) * kTcRowStride;
            if (kF32) {
                const float *fA = (const float *)sA, *fB = (const float *)sB;
                for (int s = 0; s < kn / 4; s++) {
                    const float a0 = fA[arow / 4 + s * 4 + g], a1 = fA[arow / 4 + 16 * (kTcRowStride / 4) + s * 4 + g];
#pragma unroll
                    for (int n = 0; n < NT; n++) {
                        if (n * 16 >= cout) break;
                        const float b = fB[(s * 4 + g) * wstride + n * 16 + lr];
                        if (has[0]) acc[0][n] = tc_mfma4(a0, b, acc[0][n]);
                        if (has[1]) acc[1][n] = tc_mfma4(a1, b, acc[1][n]);
                    }
                }
            } else {
                for (int s = 0; s < units / 4; s++) {
                    const int unit = s * 4 + g;
                    const uint4 a0 = *(const uint4 *)(sA + arow + unit * 16);
                    const uint4 a1 = *(const uint4 *)(sA + arow + 16 * kTcRowStride + unit * 16);
#pragma unroll
                    for (int n = 0; n < NT; n++) {
                        if (n * 16 >= cout) break;
                        const int col = n * 16 + lr;
                        const uint4 b = *(const uint4 *)(sB + col * kTcRowStride + ((unit ^ ((col >> 3) & 7)) * 16));
                        if (has[0]) acc[0][n] = tc_mfma(a0, b, acc[0][n], T());
                        if (has[1]) acc[1][n] = tc_mfma(a1, b, acc[1][n], T());
                    }
                }
            }
        }
    }
    // C / D: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < NT; n++) {
            if (n * 16 >= cout) break;
            const int col = n * 16 + lr;
            const float bv = bias ? (float)bias[col] : 0.f;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int64_t r = r0 + 32 * w + 16 * m + 4 * g + i;
                if (r < rows) out[r * cout + col] = (T)(bias ? acc[m][n][i] + bv : acc[m][n][i]);
            }
        }
}

// ---------------------------------------------------------------- the weight gradient
struct WgPlan {
    int slabs;
    int64_t slab_rows;       // a multiple of 256
};
// a function of the sizes alone: the order of every sum follows from it and from the table
WgPlan wg_plan(int64_t rows, int32_t k, int32_t cin, int32_t cout)
{
    const size_t one = (size_t)k * cin * cout * sizeof(float);
    int64_t s = std::min<int64_t>(std::max<int64_t>(d3d_divup(rows, kWgSlabRows), 1), kWgMaxSlabs);
    s = std::min<int64_t>(s, std::max<int64_t>((int64_t)(kWgPartialBytes / std::max<size_t>(one, 1)), 1));
    WgPlan p;
    p.slab_rows = d3d_divup(d3d_divup(std::max<int64_t>(rows, 1), s), 256) * 256;
    p.slabs = (int)d3d_divup(std::max<int64_t>(rows, 1), p.slab_rows);
    return p;
}

template <typename T>
__global__ __launch_bounds__(kTcThreads) void k_table_conv_wgrad(const T *__restrict__ feat, int32_t cin, const int32_t *__restrict__ table,
                                                                 int64_t rows, int32_t K, int32_t mirrored, const T *__restrict__ gout,
                                                                 int32_t cout, int64_t slab_rows, int32_t co_tiles, int32_t aligned,
                                                                 float *__restrict__ partial)
{
    constexpr bool kF32 = sizeof(T) == 4;
    constexpr int PB = kF32 ? kWgPairsF32 : kWgPairsHalf;                 // pairs of a batch
    constexpr int KS = kF32 ? 4 : 32;                                     // pairs of an MFMA
    constexpr int kSide = kF32 ? kWgPairsF32 * kWgStrideF32 * 4 : 64 * kWgStrideHalf;      // bytes of one operand's image
    __shared__ uint4 wg_smem[2 * kSide / 16];
    __shared__ int32_t sPe[kTcThreads], sPr[kTcThreads], sCnt[kTcThreads / kWave];
    char *sA = (char *)wg_smem, *sB = sA + kSide;

    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6, lr = lane & 15, g = lane >> 4;
    const int kk = (int)blockIdx.x, col = mirrored ? K - 1 - kk : kk;
    const int ci0 = ((int)blockIdx.z / co_tiles) * 64, co0 = ((int)blockIdx.z % co_tiles) * 64;
    const int cin_t = min(64, cin - ci0), cout_t = min(64, cout - co0);
    const int64_t row_begin = (int64_t)blockIdx.y * slab_rows, row_end = min(rows, row_begin + slab_rows);
    const bool al = aligned != 0;
    f32x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; n++) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int64_t base = row_begin; base < row_end; base += kTcThreads) {
        const int64_t r = base + t;
        const int32_t e = r < row_end ? table[r * K + col] : -1;
        const unsigned long long present = __ballot(e >= 0);
        if (lane == 0) sCnt[w] = __popcll(present);
        __syncthreads();
        int off = 0, n = 0;
#pragma unroll
        for (int i = 0; i < kTcThreads / kWave; i++) {
            const int c = sCnt[i];
            if (i < w) off += c;
            n += c;
        }
        if (e >= 0) {
            const int p = off + __popcll(present & ((1ull << lane) - 1ull));
            sPe[p] = e;
            sPr[p] = (int32_t)r;
        }
        __syncthreads();
        for (int p0 = 0; p0 < n; p0 += PB) {
            const int np = min(PB, n - p0), npad = (np + KS - 1) / KS * KS;
            if (kF32) {
                // row-major images [pair][channel]: A[i = channel][k = pair] and B[k = pair][j = channel] are one float per lane
                for (int u = t; u < 2 * PB * 16; u += kTcThreads) {
                    const int which = u / (PB * 16), p = (u / 16) % PB, c = u & 15;
                    if (p >= npad || c * 4 >= (which ? cout_t : cin_t)) continue;
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (p < np)
                        v = which ? tc_load16(gout + (int64_t)sPr[p0 + p] * cout + co0 + c * 4, al)
                                  : tc_load16(feat + (int64_t)sPe[p0 + p] * cin + ci0 + c * 4, al);
                    *(uint4 *)((which ? sB : sA) + ((size_t)p * kWgStrideF32 + c * 4) * 4) = v;
                }
            } else {
                // transposed images [channel][pair]: thread -> (operand, 8 pairs, 8 channels)
                const int which = t >> 7, pb = (t >> 3) & 15, cb = t & 7;
                if (pb * 8 < npad && cb * 8 < (which ? cout_t : cin_t)) {
                    uint4 in[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const int p = pb * 8 + i;
                        in[i] = make_uint4(0, 0, 0, 0);
                        if (p < np)
                            in[i] = which ? tc_load16(gout + (int64_t)sPr[p0 + p] * cout + co0 + cb * 8, al)
                                          : tc_load16(feat + (int64_t)sPe[p0 + p] * cin + ci0 + cb * 8, al);
                    }
                    char *dst = which ? sB : sA;
#pragma unroll
                    for (int j = 0; j < 8; j++) *(uint4 *)(dst + (cb * 8 + j) * kWgStrideHalf + ((pb ^ cb) * 16)) = tc_column(in, j);
                }
            }
            __syncthreads();
            if (16 * w < cin_t) {
                if (kF32) {
                    const float *fA = (const float *)sA, *fB = (const float *)sB;
                    for (int s = 0; s < npad / 4; s++) {
                        const float a = fA[(s * 4 + g) * kWgStrideF32 + 16 * w + lr];
#pragma unroll
                        for (int nt = 0; nt < 4; nt++) {
                            if (nt * 16 >= cout_t) break;
                            acc[nt] = tc_mfma4(a, fB[(s * 4 + g) * kWgStrideF32 + nt * 16 + lr], acc[nt]);
                        }
                    }
                } else {
                    for (int s = 0; s < npad / 32; s++) {
                        const int unit = s * 4 + g, ch = 16 * w + lr;
                        const uint4 a = *(const uint4 *)(sA + ch * kWgStrideHalf + ((unit ^ ((ch >> 3) & 7)) * 16));
#pragma unroll
                        for (int nt = 0; nt < 4; nt++) {
                            if (nt * 16 >= cout_t) break;
                            const int cj = nt * 16 + lr;
                            const uint4 b = *(const uint4 *)(sB + cj * kWgStrideHalf + ((unit ^ ((cj >> 3) & 7)) * 16));
                            acc[nt] = tc_mfma(a, b, acc[nt], T());
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    if (16 * w < cin_t) {
        float *dst = partial + ((int64_t)blockIdx.y * K + kk) * cin * cout;
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
            if (nt * 16 >= cout_t) break;
#pragma unroll
            for (int i = 0; i < 4; i++) dst[(int64_t)(ci0 + 16 * w + 4 * g + i) * cout + co0 + nt * 16 + lr] = acc[nt][i];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kTcThreads) void k_table_conv_fold(const float *__restrict__ partial, int64_t n, int32_t slabs, T *__restrict__ gw)
{
    const int64_t i = (int64_t)blockIdx.x * kTcThreads + threadIdx.x;
    if (i >= n) return;
    float s = partial[i];
    for (int k = 1; k < slabs; k++) s += partial[(int64_t)k * n + i];     // ascending slabs: the same bits on every run
    gw[i] = (T)s;
}

bool tc_channels_ok(int32_t c) { return c >= 16 && c <= 256 && c % 16 == 0; }

// D3D_OK when the sizes and the dtype are served, the refusal otherwise (nothing touched either way)
int tc_check(int64_t src_rows, int32_t cin, int64_t rows, int32_t k, int32_t cout, int32_t dtype)
{
    if (src_rows < 0 || rows < 0 || k < 1 || cin < 1 || cout < 1) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64 && dtype != D3D_F16 && dtype != D3D_BF16) return D3D_ERR_BAD_ARG;
    if (dtype == D3D_F64 || !tc_channels_ok(cin) || !tc_channels_ok(cout) || k > 343 || rows > kRowMax || src_rows > kRowMax)
        return D3D_ERR_UNSUPPORTED;
    return D3D_OK;
}

}  // namespace

extern "C" int d3d_table_conv(const void *feat, int64_t src_rows, int32_t cin, const int32_t *table, int64_t rows, int32_t k,
                              int32_t mirrored, const void *weight, const void *bias, int32_t cout, int32_t dtype, void *out, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int rc = tc_check(src_rows, cin, rows, k, cout, dtype);
    if (rc != D3D_OK) return rc;
    if (rows == 0) return D3D_OK;
    if (!table || !out || !weight || (src_rows > 0 && !feat)) return D3D_ERR_BAD_ARG;
    const int32_t al = row_aligned16(feat) && row_aligned16(weight);
    return dispatch_dtype<D3D_F32, D3D_F16, D3D_BF16>(dtype, [&](auto p) {
        typedef typename decltype(p)::T T;
        const int nt = cout <= 16 ? 1 : cout <= 32 ? 2 : cout <= 64 ? 4 : cout <= 128 ? 8 : 16;
        return dispatch_int<1, 2, 4, 8, 16>(nt, [&](auto ntc) {
            constexpr int NT = decltype(ntc)::value;
            D3D_LAUNCH("k_table_conv", (k_table_conv<T, NT>), dim3((unsigned)d3d_divup(rows, kTcTile)), dim3(kTcThreads),
                       tc_lds_bytes<T>(cout), st, (const T *)feat, cin, table, rows, k, mirrored, (const T *)weight, (const T *)bias, cout,
                       al, (T *)out);
            return D3D_OK;
        });
    });
}

extern "C" size_t d3d_table_conv_wgrad_workspace_bytes(int64_t rows, int32_t k, int32_t cin, int32_t cout)
{
    if (rows < 1 || rows > kRowMax || k < 1 || k > 343 || !tc_channels_ok(cin) || !tc_channels_ok(cout)) return 0;
    return d3d_align_up((size_t)wg_plan(rows, k, cin, cout).slabs * k * cin * cout * sizeof(float));
}

extern "C" int d3d_table_conv_wgrad(const void *feat, int64_t src_rows, int32_t cin, const int32_t *table, int64_t rows, int32_t k,
                                    int32_t mirrored, const void *grad_out, int32_t cout, int32_t dtype, void *grad_weight,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int rc = tc_check(src_rows, cin, rows, k, cout, dtype);
    if (rc != D3D_OK) return rc;
    if (!grad_weight) return D3D_ERR_BAD_ARG;
    const int64_t n = (int64_t)k * cin * cout;
    if (rows == 0) {                                                      // an empty sum
        D3D_HIP_CHECK(hipMemsetAsync(grad_weight, 0, (size_t)n * (dtype == D3D_F32 ? 4 : 2), st));
        return D3D_OK;
    }
    if (!table || !grad_out || (src_rows > 0 && !feat)) return D3D_ERR_BAD_ARG;
    if (!workspace || workspace_bytes < d3d_table_conv_wgrad_workspace_bytes(rows, k, cin, cout)) return D3D_ERR_WORKSPACE;
    const WgPlan plan = wg_plan(rows, k, cin, cout);
    const int32_t al = row_aligned16(feat) && row_aligned16(grad_out);
    const int ci_tiles = (cin + 63) / 64, co_tiles = (cout + 63) / 64;
    return dispatch_dtype<D3D_F32, D3D_F16, D3D_BF16>(dtype, [&](auto p) {
        typedef typename decltype(p)::T T;
        D3D_LAUNCH("k_table_conv_wgrad", (k_table_conv_wgrad<T>), dim3((unsigned)k, (unsigned)plan.slabs, (unsigned)(ci_tiles * co_tiles)),
                   dim3(kTcThreads), 0, st, (const T *)feat, cin, table, rows, k, mirrored, (const T *)grad_out, cout, plan.slab_rows,
                   co_tiles, al, (float *)workspace);
        D3D_LAUNCH("k_table_conv_fold", (k_table_conv_fold<T>), dim3((unsigned)d3d_divup(n, kTcThreads)), dim3(kTcThreads), 0, st,
                   (const float *)workspace, n, plan.slabs, (T *)grad_weight);
        return D3D_OK;
    });
}
