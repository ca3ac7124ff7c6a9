// assign.hip -- the association steps of the reference's tracker on MI355X (gfx950).
// Replaces HungarianMatcher.match (reference d3d/tracking/matcher.pyx:188-230, which calls scipy.optimize.linear_sum_assignment
// once per class) and NearestNeighborMatcher.match (:164-186 + BaseMatcher.match_by_order :90-121).
//
// LSAP (k_lsap): scipy's solver, step for step -- the shortest augmenting path method of Crouse (2016), scipy's
// rectangular_lsap.cpp.  A tall problem is solved transposed; rows are taken in order from u = v = 0; each row runs a
// Dijkstra search over the columns still "remaining", then the duals are updated and the path is augmented.  Everything is
// fp64 and every expression is evaluated in scipy's order (-ffp-contract=off), so the duals -- and the choices they drive --
// are the same bits.  The one sequential rule that a parallel argmin must reproduce is scipy's choice of the column of least
// reduced cost: it scans `remaining` (nc-1 .. 0 at the start of each row; a column is removed by moving the last entry into its
// place) and keeps the first strict minimum, except that an UNASSIGNED column of equal cost replaces the current choice.  So
// among the columns of the least cost, the last unassigned one in `remaining` order wins, else the first assigned one -- a
// total order on (cost, key) with key = nc-1-pos for an unassigned column and nc+pos for an assigned one, pos = its place in
// `remaining`.  One workgroup per problem; thread t owns the columns t, t+T, ...: every per-column quantity (shortest path
// cost, dual v, path, row4col, pos, visited) is touched by its owner only, and the swap-removal is applied by the owner of
// the column that moves (it sees pos == the new size).  A step is: each owner relaxes its columns from row i (coalesced reads
// of the cost row), a wave argmin by shuffles, one LDS slot per wave, ONE barrier, and every thread reduces the slots itself.
// The row duals u live in LDS (or the workspace) and are updated by the owners of the visited columns: SR minus the current
// row is exactly {row4col[j] : j visited, j assigned}.
//
// Nearest neighbour (k_nn_propose + k_nn_rounds): match_by_order over the pairs sorted by (distance, src position, dst
// position) -- a strict total order on the acceptable pairs -- is the greedy matching of that order.  It equals the matching
// built by taking LOCALLY DOMINANT pairs, i.e. pairs that are the least acceptable pair at their row AND at their column among
// the still-free rows and columns: such a pair e is taken by the greedy (every pair that could block it touches its row or
// column, so it is larger and comes later), and the greedy on the whole set is e plus the greedy on the set without e's row
// and column (the pairs before e do not touch them; the pairs after e that do are blocked by e).  Vertex-disjoint locally
// dominant pairs can be taken together.  So: every free row points at its least free acceptable column, every free column at
// its least free acceptable row; the mutual pairs are matched in one round; the pointers that point at a side matched in the
// round are rebuilt.  The least acceptable free pair is always mutual, so a round without a match means none is left and a
// round matches at least one pair: at most min(ns, nd) + 1 rounds (one per pair in the worst case, a chain of decreasing pairs).
#include "common.hpp"
#include <math.h>

namespace {

constexpr int32_t kLsapInvalid = 1;        // status bit: a NaN or -inf entry (scipy: "matrix contains invalid numeric entries")
constexpr int32_t kLsapInfeasible = 2;     // status bit: a row without a finite path (scipy: "cost matrix is infeasible")
constexpr int32_t kLsapTooBig = 4;         // status bit: a problem larger than the max_rows / max_cols the caller stated, or
                                           // whose state runs past the workspace

struct Best {
    double c;
    int s, j, row;
};

__device__ __forceinline__ bool best_less(const Best &a, const Best &b) { return a.c < b.c || (a.c == b.c && a.s < b.s); }

__device__ __forceinline__ Best wave_min(Best b)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        Best x;
        x.c = __shfl_xor(b.c, o, kWave);
        x.s = __shfl_xor(b.s, o, kWave);
        x.j = __shfl_xor(b.j, o, kWave);
        x.row = __shfl_xor(b.row, o, kWave);
        if (best_less(x, b)) b = x;
    }
    return b;
}

// per-problem state: doubles spc[nc], v[nc], u[nr]; ints path[nc], row4col[nc], pos[nc], seen[nc], col4row[nr]
__host__ __device__ inline size_t lsap_state_bytes(int64_t nr, int64_t nc) { return (size_t)(nc * 2 + nr) * 8 + (size_t)(nc * 4 + nr) * 4; }

// one workgroup per problem b: rows row_idx[row_off[b] ..], columns col_idx[col_off[b] ..] of cost (leading dimension ld).
// row_match[row_off[b] + r] <- the problem's column matched to row r or -1, col_match[col_off[b] + c] likewise.
template <class T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_lsap(const T *__restrict__ cost, int64_t ld, const int64_t *__restrict__ row_idx,
                                                const int64_t *__restrict__ col_idx, const int64_t *__restrict__ row_off,
                                                const int64_t *__restrict__ col_off, int64_t max_rows, int64_t max_cols,
                                                int32_t *row_match, int32_t *col_match, int32_t *status, char *ws_global, size_t ws_bytes,
                                                int use_lds)
{
    constexpr int NW = BLOCK / kWave;
    extern __shared__ __align__(16) char lds[];
    __shared__ Best slot[2][NW];
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const int64_t b = blockIdx.x;
    const int64_t ro = row_off[b], co = col_off[b];
    const int64_t NR = row_off[b + 1] - ro, NC = col_off[b + 1] - co;      // the problem as given
    for (int64_t r = tid; r < NR; r += BLOCK) row_match[ro + r] = -1;
    for (int64_t c = tid; c < NC; c += BLOCK) col_match[co + c] = -1;
    if (NR == 0 || NC == 0) return;
    if (NR > max_rows || NC > max_cols || (!use_lds && (size_t)(ro + co + NR + NC) * 32 > ws_bytes)) {
        if (tid == 0) atomicOr(status, kLsapTooBig);
        return;
    }
    const bool tr = NC < NR;                                   // tall: solve the transpose (rows <-> columns)
    const int64_t nr = tr ? NC : NR, nc = tr ? NR : NC;
    const int64_t *kr_idx = tr ? col_idx + co : row_idx + ro;  // the solver's rows / columns as indices into cost
    const int64_t *kc_idx = tr ? row_idx + ro : col_idx + co;
    // cost of the solver's (i, j): cost[kr_idx[i] * ld + kc_idx[j]] untransposed, cost[kc_idx[j] * ld + kr_idx[i]] transposed
    const int64_t rs = tr ? 1 : ld, cs = tr ? ld : 1;

    // scipy tests the whole matrix for NaN and -inf before it solves anything
    if (tid == 0) bad = 0;
    __syncthreads();
    {
        int mybad = 0;
        const int64_t total = nr * nc;
        for (int64_t e0 = tid; e0 < total; e0 += 4 * BLOCK) {      // four loads in flight per thread
            double c[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int64_t e = e0 + u * BLOCK, ec = e < total ? e : total - 1;
                const int64_t i = ec / nc, j = ec - i * nc;
                c[u] = (double)cost[kr_idx[i] * rs + kc_idx[j] * cs];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) mybad |= (c[u] != c[u]) | (c[u] == -INFINITY);
        }
        if (mybad) bad = 1;
    }
    __syncthreads();
    if (bad) {
        if (tid == 0) atomicOr(status, kLsapInvalid);
        return;
    }

    char *base = use_lds ? lds : ws_global + (size_t)(ro + co) * 32;
    double *spc = (double *)base, *v = spc + nc, *u = v + nc;
    int32_t *path = (int32_t *)(u + nr), *row4col = path + nc, *pos = row4col + nc, *seen = pos + nc, *col4row = seen + nc;
    for (int64_t j = tid; j < nc; j += BLOCK) { v[j] = 0.0; path[j] = -1; row4col[j] = -1; }
    for (int64_t i = tid; i < nr; i += BLOCK) { u[i] = 0.0; col4row[i] = -1; }
    __syncthreads();

    int buf = 0;
    for (int64_t cur = 0; cur < nr; cur++) {
        for (int64_t j = tid; j < nc; j += BLOCK) { spc[j] = INFINITY; seen[j] = 0; pos[j] = (int32_t)(nc - 1 - j); }
        int64_t i = cur;
        double minVal = 0.0;
        int64_t R = nc;                       // entries left in `remaining`
        int last_j = -1, last_pos = -1;       // the previous step's pick: its owner marks it seen, the column at pos R moves there
        int sink = -1;
        while (sink < 0) {
            const double ui = u[i];
            const T *crow = cost + kr_idx[i] * rs;
            Best best = {INFINITY, 0x7fffffff, -1, -1};
            for (int64_t j = tid; j < nc; j += BLOCK) {
                if (seen[j]) continue;
                if (j == last_j) { seen[j] = 1; continue; }
                int p = pos[j];
                if (p == R) { p = last_pos; pos[j] = p; }
                const double c = (double)crow[kc_idx[j] * cs];
                const double r = minVal + c - ui - v[j];
                double sj = spc[j];
                if (r < sj) { path[j] = (int32_t)i; spc[j] = r; sj = r; }
                const int rw = row4col[j];
                const Best cand = {sj, rw == -1 ? (int)(nc - 1 - p) : (int)(nc + p), (int)j, rw};
                if (best_less(cand, best)) best = cand;
            }
            best = wave_min(best);
            if (NW > 1) {
                if (lane == 0) slot[buf][w] = best;
                __syncthreads();
                best = slot[buf][0];
#pragma unroll
                for (int k = 1; k < NW; k++)
                    if (best_less(slot[buf][k], best)) best = slot[buf][k];
                buf ^= 1;
            }
            minVal = best.c;
            if (!(minVal < INFINITY)) {               // no finite path from this row: scipy's RECTANGULAR_LSAP_INFEASIBLE
                if (tid == 0) atomicOr(status, kLsapInfeasible);
                return;
            }
            if (best.row == -1) sink = best.j;
            else i = best.row;
            last_j = best.j;
            last_pos = best.s < nc ? (int)(nc - 1 - best.s) : (int)(best.s - nc);
            R--;
        }
        // duals: u[i] += minVal - spc[col4row[i]] for the visited rows but `cur`, v[j] -= minVal - spc[j] for the visited columns
        for (int64_t j = tid; j < nc; j += BLOCK) {
            if (!seen[j] && j != last_j) continue;
            const double d = minVal - spc[j];
            v[j] -= d;
            const int rw = row4col[j];
            if (rw != -1) u[rw] += d;
        }
        __syncthreads();
        if (tid == 0) {
            u[cur] += minVal;
            int64_t j = sink;                         // augment along the path
            for (;;) {
                const int64_t ii = path[j];
                row4col[j] = (int32_t)ii;
                const int64_t nj = col4row[ii];
                col4row[ii] = (int32_t)j;
                j = nj;
                if (ii == cur) break;
            }
        }
        __syncthreads();
    }
    // solver column j holds solver row row4col[j] (every solver row is assigned)
    for (int64_t j = tid; j < nc; j += BLOCK) {
        const int rw = row4col[j];
        if (rw < 0) continue;
        if (tr) { row_match[ro + j] = rw; col_match[co + rw] = (int32_t)j; }
        else { row_match[ro + rw] = (int32_t)j; col_match[co + j] = rw; }
    }
}

// ------------------------------------------------------------------------------------------------ nearest neighbour greedy
__device__ __forceinline__ uint32_t f32_order(float d)
{
    const uint32_t u = __float_as_uint(d + 0.0f);            // (-0 -> +0: equal distances compare equal)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct NNArgs {
    const float *dist;
    int64_t ld;
    const int64_t *src_idx, *dst_idx;
    const int32_t *src_tag, *dst_tag;
    const float *dst_thr;
    const uint8_t *src_free, *dst_free;        // NULL = all free
    int64_t ns, nd;
    int32_t *src_match, *dst_match;
    int32_t *prop;                             // [ns] row r's least free acceptable column, -1 = none
    unsigned long long *colkey;                // [nd] (order(distance) << 32 | row) of column c's least free acceptable row, ~0 = none
    int32_t *rescan;                           // [ns + nd] rows (r) and columns (-1 - c) whose pointer went stale
};

__device__ __forceinline__ int32_t ld_i32(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the least free acceptable column of row r by (distance, column), one wavefront; -1 if none
__device__ int nn_row_best(const NNArgs &a, int64_t r, int lane)
{
    const int32_t tag = a.src_tag[r];
    const float *drow = a.dist + a.src_idx[r] * a.ld;
    uint32_t bk = 0xffffffffu;
    int bj = 0x7fffffff;
    for (int64_t j = lane; j < a.nd; j += kWave) {
        if (a.dst_tag[j] != tag) continue;
        if (a.dst_free && !a.dst_free[j]) continue;
        if (ld_i32(&a.dst_match[j]) >= 0) continue;
        const float d = drow[a.dst_idx[j]];
        if (!(d <= a.dst_thr[j])) continue;
        const uint32_t k = f32_order(d);
        if (k < bk) { bk = k; bj = (int)j; }             // (j ascending per lane: the first of equal keys is kept)
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const uint32_t ok = __shfl_xor(bk, o, kWave);
        const int oj = __shfl_xor(bj, o, kWave);
        if (ok < bk || (ok == bk && oj < bj)) { bk = ok; bj = oj; }
    }
    return bj == 0x7fffffff ? -1 : bj;
}

// the least free acceptable row of column c by (distance, row), one wavefront, as a key (~0 if none)
__device__ unsigned long long nn_col_best(const NNArgs &a, int64_t c, int lane)
{
    const int32_t tag = a.dst_tag[c];
    const float thr = a.dst_thr[c];
    const int64_t col = a.dst_idx[c];
    unsigned long long bk = ~0ull;
    for (int64_t r = lane; r < a.ns; r += kWave) {
        if (a.src_tag[r] != tag) continue;
        if (a.src_free && !a.src_free[r]) continue;
        if (ld_i32(&a.src_match[r]) >= 0) continue;
        const float d = a.dist[a.src_idx[r] * a.ld + col];
        if (!(d <= thr)) continue;
        const unsigned long long k = ((unsigned long long)f32_order(d) << 32) | (unsigned long long)r;
        if (k < bk) bk = k;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(bk, o, kWave);
        if (ok < bk) bk = ok;
    }
    return bk;
}

// the rows' pointers at the start: a wavefront per row
__global__ __launch_bounds__(256) void k_nn_propose(NNArgs a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = (int64_t)blockIdx.x * (256 / kWave) + (threadIdx.x >> 6);
    if (r >= a.ns) return;
    const bool free_ = !a.src_free || a.src_free[r];
    const int p = free_ ? nn_row_best(a, r, lane) : -1;
    if (lane == 0) a.prop[r] = p;
}

// the columns' pointers at the start: thread = column (adjacent lanes read adjacent columns of a row), workgroup row y = a chunk
// of `chunk` rows; the least key of the chunk goes to the column's key by one atomicMin (colkey preset to ~0)
constexpr int64_t kNNChunk = 64;
__global__ __launch_bounds__(256) void k_nn_propose_cols(NNArgs a, int64_t chunk)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.nd || (a.dst_free && !a.dst_free[c])) return;
    const int32_t tag = a.dst_tag[c];
    const float thr = a.dst_thr[c];
    const int64_t col = a.dst_idx[c];
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < a.ns ? r0 + chunk : a.ns;
    unsigned long long bk = ~0ull;
    for (int64_t r = r0; r < r1; r++) {
        if (a.src_tag[r] != tag || (a.src_free && !a.src_free[r])) continue;
        const float d = a.dist[a.src_idx[r] * a.ld + col];
        if (!(d <= thr)) continue;
        const unsigned long long k = ((unsigned long long)f32_order(d) << 32) | (unsigned long long)r;
        if (k < bk) bk = k;
    }
    if (bk != ~0ull) atomicMin(&a.colkey[c], bk);
}

constexpr int kNNThreads = 1024;

// rounds of mutual picks in one workgroup: match every row whose column points back at it, then rebuild the pointers that
// point at a side matched in this round; stop after a round without a match
__global__ __launch_bounds__(kNNThreads) void k_nn_rounds(NNArgs a)
{
    __shared__ int matched, nres;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
    for (;;) {
        if (tid == 0) { matched = 0; nres = 0; }
        __syncthreads();
        for (int64_t r = tid; r < a.ns; r += kNNThreads) {
            const int p = ld_i32(&a.prop[r]);
            if (p < 0 || ld_i32(&a.src_match[r]) >= 0) continue;
            const unsigned long long k = __hip_atomic_load(&a.colkey[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k != ~0ull && (int64_t)(k & 0xffffffffu) == r) {
                __hip_atomic_store(&a.src_match[r], (int32_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&a.dst_match[p], (int32_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                atomicOr(&matched, 1);
            }
        }
        __threadfence();
        __syncthreads();
        if (!matched) break;                   // no acceptable free pair is left (the least one would have been mutual)
        // stale pointers: a free row whose column was matched, a free column whose row was matched
        for (int64_t r = tid; r < a.ns; r += kNNThreads) {
            const int p = ld_i32(&a.prop[r]);
            if (p >= 0 && ld_i32(&a.src_match[r]) < 0 && ld_i32(&a.dst_match[p]) >= 0)
                __hip_atomic_store(&a.rescan[atomicAdd(&nres, 1)], (int32_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (int64_t c = tid; c < a.nd; c += kNNThreads) {
            const unsigned long long k = __hip_atomic_load(&a.colkey[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k != ~0ull && ld_i32(&a.dst_match[c]) < 0 && ld_i32(&a.src_match[k & 0xffffffffu]) >= 0)
                __hip_atomic_store(&a.rescan[atomicAdd(&nres, 1)], (int32_t)(-1 - c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence();
        __syncthreads();
        const int n = nres;
        for (int k = w; k < n; k += kNNThreads / kWave) {
            const int32_t e = ld_i32(&a.rescan[k]);
            if (e >= 0) {
                const int p = nn_row_best(a, e, lane);
                if (lane == 0) __hip_atomic_store(&a.prop[e], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                const unsigned long long key = nn_col_best(a, -1 - (int64_t)e, lane);
                if (lane == 0) __hip_atomic_store(&a.colkey[-1 - (int64_t)e], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __threadfence();
        __syncthreads();
    }
}

}  // namespace

extern "C" size_t d3d_lsap_batched_workspace_bytes(int64_t batches, int64_t total_rows, int64_t total_cols)
{
    if (batches < 1) batches = 1;
    if (total_rows < 0) total_rows = 0;
    if (total_cols < 0) total_cols = 0;
    return d3d_align_up((size_t)(total_rows + total_cols) * 32) + 256;
}

extern "C" int d3d_lsap_batched(const void *cost, int32_t dtype, int64_t ld, const int64_t *row_idx, const int64_t *col_idx,
                                const int64_t *row_off, const int64_t *col_off, int64_t batches, int64_t max_rows, int64_t max_cols,
                                int32_t *row_match, int32_t *col_match, int32_t *status, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (batches < 0 || max_rows < 0 || max_cols < 0 || ld < 0 || !status) return D3D_ERR_BAD_ARG;
    if (dtype != D3D_F32 && dtype != D3D_F64) return D3D_ERR_BAD_ARG;
    D3D_HIP_CHECK(hipMemsetAsync(status, 0, 4, st));
    if (batches == 0) return D3D_OK;
    if (!row_off || !col_off || batches > 0x7fffffff) return D3D_ERR_BAD_ARG;
    if (max_rows >= (1ll << 30) || max_cols >= (1ll << 30)) return D3D_ERR_BAD_ARG;
    if (max_rows > 0 && max_cols > 0 && (!cost || !row_idx || !col_idx || !row_match || !col_match)) return D3D_ERR_BAD_ARG;
    if ((max_rows > 0 && !row_match) || (max_cols > 0 && !col_match)) return D3D_ERR_BAD_ARG;
    // the solver's larger side is its columns; LDS holds one problem's state when it fits
    const int64_t kc = max_rows > max_cols ? max_rows : max_cols, kr = max_rows < max_cols ? max_rows : max_cols;
    const size_t state = lsap_state_bytes(kr, kc);
    const bool use_lds = state <= 48 * 1024;
    if (!use_lds && !workspace) return D3D_ERR_WORKSPACE;      // (a problem whose state would run past it sets kLsapTooBig)
    const size_t lds = use_lds ? state : 0;
    const unsigned grid = (unsigned)batches;
    auto go = [&](auto prec) {
        typedef typename decltype(prec)::T T;
        const T *c = (const T *)cost;
        return dispatch_int<kWave, 256, 1024>(kc <= kWave ? kWave : kc <= 2048 ? 256 : 1024, [&](auto block) {
            D3D_LAUNCH("k_lsap", (k_lsap<T, block>), dim3(grid), dim3(block), lds, st, c, ld, row_idx, col_idx, row_off, col_off,
                       max_rows, max_cols, row_match, col_match, status, (char *)workspace, workspace_bytes, (int)use_lds);
            return D3D_OK;
        });
    };
    return dispatch_dtype<D3D_F32, D3D_F64>(dtype, go);
}

// the scratch arrays of NNArgs, from its ns and nd
static void nn_carve(WsCarver &w, NNArgs &a)
{
    a.prop = w.take<int32_t>((size_t)a.ns);
    a.rescan = w.take<int32_t>((size_t)(a.ns + a.nd));
    a.colkey = w.take<unsigned long long>((size_t)a.nd);
}

extern "C" size_t d3d_nn_match_workspace_bytes(int64_t ns, int64_t nd)
{
    NNArgs a;
    a.ns = ns < 1 ? 1 : ns;
    a.nd = nd < 1 ? 1 : nd;
    WsCarver w(nullptr, 0);
    nn_carve(w, a);
    return w.off;
}

extern "C" int d3d_nn_match(const float *dist, int64_t ld, const int64_t *src_idx, int64_t ns, const int64_t *dst_idx, int64_t nd,
                            const int32_t *src_tag, const int32_t *dst_tag, const float *dst_threshold, const uint8_t *src_free,
                            const uint8_t *dst_free, int32_t *src_match, int32_t *dst_match, void *workspace, size_t workspace_bytes,
                            void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (ns < 0 || nd < 0 || ld < 0 || ns >= (1ll << 31) || nd >= (1ll << 31)) return D3D_ERR_BAD_ARG;
    if ((ns > 0 && !src_match) || (nd > 0 && !dst_match)) return D3D_ERR_BAD_ARG;
    if (ns > 0) D3D_HIP_CHECK(hipMemsetAsync(src_match, 0xff, (size_t)ns * 4, st));
    if (nd > 0) D3D_HIP_CHECK(hipMemsetAsync(dst_match, 0xff, (size_t)nd * 4, st));
    if (ns == 0 || nd == 0) return D3D_OK;
    if (!dist || !src_idx || !dst_idx || !src_tag || !dst_tag || !dst_threshold) return D3D_ERR_BAD_ARG;
    WsCarver w(workspace, workspace_bytes);
    NNArgs a;
    a.dist = dist; a.ld = ld; a.src_idx = src_idx; a.dst_idx = dst_idx; a.src_tag = src_tag; a.dst_tag = dst_tag;
    a.dst_thr = dst_threshold; a.src_free = src_free; a.dst_free = dst_free; a.ns = ns; a.nd = nd;
    a.src_match = src_match; a.dst_match = dst_match;
    nn_carve(w, a);
    if (!workspace || !w.ok()) return D3D_ERR_WORKSPACE;
    D3D_HIP_CHECK(hipMemsetAsync(a.colkey, 0xff, (size_t)nd * 8, st));
    D3D_LAUNCH("k_nn_propose", k_nn_propose, dim3((unsigned)d3d_divup(ns, 256 / kWave)), dim3(256), 0, st, a);
    const int64_t chunk = ns > kNNChunk * 65535 ? d3d_divup(ns, 65535) : kNNChunk;        // (grid.y <= 65535)
    D3D_LAUNCH("k_nn_propose_cols", k_nn_propose_cols, dim3((unsigned)d3d_divup(nd, 256), (unsigned)d3d_divup(ns, chunk)), dim3(256), 0,
               st, a, chunk);
    D3D_LAUNCH("k_nn_rounds", k_nn_rounds, dim3(1), dim3(kNNThreads), 0, st, a);
    return D3D_OK;
}
