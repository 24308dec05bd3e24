// Rank (Spearman) IC (include/afm_rankic.h): DataFrame.corr(method='spearman') per date for the
// analyzer's signal or the K columns of a factor screen, bit for bit.  The Pearson IC is one
// sequential Welford chain per (date, column); the Spearman sums are sums of small integers
// (doubled ranks minus n + 1), exact in any order, so everything here is parallel: a sort, two
// binary searches per row, and a workgroup reduction in int64.
//
//  rank_returns_kernel  one workgroup per (evaluated date, return): the doubled average ranks of
//                       the demeaned return over the date's compacted rows, their sum of squares,
//                       and whether the return is finite on every row -- once per date, shared by
//                       every column.
//  rank_ic_kernel       one workgroup per (date, column): the column's values gathered through
//                       rows_idx (z-scored on the way when zs is given), their order-preserving
//                       8-byte keys sorted -- keys only; no index travels through the sort -- and
//                       every row then finds the lower and upper bound of its own key:
//                       2 * rank = lb + ub + 1.  Row e pairs with rrank[q][t][e] by a coalesced
//                       read.  A date whose returns are not all finite, or a column with a
//                       non-finite value on the date, takes the masked path: per return, pandas'
//                       rule with up to two masked rankings (an excluded row sorts as the pad key).
//
// The sort and the searches are afm_order.h's run sort: the rows of a date in runs, each a bitonic
// network in LDS over a power of two (9,371 rows: 8192 + 1179 padded to 2048, less than half the
// compare-exchanges of one network over 16384), a row's bounds the sums of its bounds in every
// run (xs_rank_kernel's scheme).  A date of up to kRankLdsRows rows keeps its runs side by side in
// LDS; a longer one (up to kRankMaxRows) writes each sorted run to the workgroup's slot of the
// caller's scratch and searches there.  The grid is then capped at kRankSlots workgroups, each
// looping over its items, so the scratch is kRankSlots * lda words.
#include "afm_internal.h"
#include "afm_rankic.h"

#pragma clang fp contract(off)

#include "afm_np_sum.h"                // qnan
#include "afm_order.h"                 // okey, sort_rows, bounds

namespace afm {
namespace {

constexpr int kRankThreads = 1024;     // 16 waves
constexpr int kRankMaxRows = 32768;    // afm_xs_prepare_f64's limit
constexpr int kRankPer = kRankMaxRows / kRankThreads;   // rows per thread (masked path registers)
constexpr int kRankSlots = 1024;       // workgroups of a launch that uses the scratch
// the entry points' own limits (the scratch is needed past kRankLdsRows rows; the tests shape
// their dates by both): afm_order.h's, restated
constexpr int kRankLdsRows = 16384;
constexpr int kRankChunk = 16384;
static_assert(kRankThreads == kSortThreads, "afm_order.h's sort is written for this workgroup");
static_assert(kRankLdsRows == kSortLdsRows && kRankChunk == kSortChunk, "afm_order.h's run sort");

// 2 * (average rank) of key k (< kSortPad) among the sorted keys below the pad
__device__ __forceinline__ int rank2(const u64* lds, const u64* scr, int n, u64 k) {
    int lb, ub;
    bounds(lds, scr, n, k, lb, ub);
    return 1 + lb + ub;
}

// the sum of v over the workgroup (exact: integers), on every thread
__device__ i64 block_sum(i64 v, i64* sred) {
    const int tid = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) sred[tid >> 6] = v;
    __syncthreads();
    i64 s = 0;
#pragma unroll
    for (int w = 0; w < kRankThreads / 64; ++w) s += sred[w];
    return s;
}

// pandas' last two lines: sums in doubled units (4 * the sums of nancorr_spearman), exact
__device__ __forceinline__ double spearman_finish(i64 sxy, i64 sxx, i64 syy) {
    const double div = __builtin_sqrt(((double)sxx / 4.0) * ((double)syy / 4.0));
    return div != 0 ? ((double)sxy / 4.0) / div : qnan();
}

// ---- the return ranks of a date ----------------------------------------------------------------
struct RankRetArgs {
    int64_t T, lda;
    const int32_t* dates;     // [nd]
    int64_t items;            // nd * 3
    const double* rows;       // [4][T][lda]
    const int32_t* nrows;     // [T]
    int32_t* rrank;           // [3][T][lda]
    i64* rsum;                // [T][3]
    u64* scratch;             // [gridDim.x][lda] when lda > kRankLdsRows
};

__global__ __launch_bounds__(kRankThreads) void rank_returns_kernel(RankRetArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ i64 sred[kRankThreads / 64];
    u64* lds = reinterpret_cast<u64*>(dyn);
    u64* scr = g.scratch ? g.scratch + (int64_t)blockIdx.x * g.lda : nullptr;
    const int tid = threadIdx.x;
    const int64_t plane = g.T * g.lda;
    for (int64_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const int q = (int)(item % 3);
        const int64_t t = g.dates[item / 3];
        const int n = min(max(g.nrows[t], 0), (int)g.lda);
        const double* R = g.rows + (1 + q) * plane + t * g.lda;
        int32_t* out = g.rrank + q * plane + t * g.lda;
        int fin = 1;
        for (int e = tid; e < n; e += kRankThreads) fin &= __builtin_isfinite(R[e]);
        const bool all_fin = __syncthreads_and(fin);
        sort_rows(lds, scr, n, [&](int e) { return okey(R[e]); });
        i64 syy = 0;
        for (int e = tid; e < n; e += kRankThreads) {
            const int r2 = rank2(lds, scr, n, okey(R[e]));
            out[e] = r2;
            const i64 dy = r2 - (n + 1);
            syy += dy * dy;
        }
        syy = block_sum(syy, sred);
        if (tid == 0) g.rsum[t * 3 + q] = all_fin ? syy : -1;
    }
}

// ---- the rank IC of every (date, column) -----------------------------------------------------------
struct RankIcArgs {
    const double* base;       // plane k: base + cols[k] * col_stride, [T][lda]
    int64_t col_stride, T, lda;
    const int32_t* cols;      // [K]
    int K;
    const double* zs;         // [..][lda][2] {mu, 1/sd}, or null: raw values
    const int32_t* zcols;     // [K] zs row of each column (null: row k)
    const int32_t* dates;     // [nd]
    int64_t items;            // nd * K
    const double* rows;       // [4][T][lda]: planes 1..3 the demeaned returns
    const int32_t* rows_idx;  // [T][lda]
    const int32_t* nrows;     // [T]
    const int32_t* rrank;     // [3][T][lda]
    const i64* rsum;          // [T][3]
    u64* scratch;             // [gridDim.x][lda] when lda > kRankLdsRows
    double* ic;               // [nd][K][3]
};

template <bool Z>
__global__ __launch_bounds__(kRankThreads) void rank_ic_kernel(RankIcArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ i64 sred[kRankThreads / 64];
    u64* lds = reinterpret_cast<u64*>(dyn);
    u64* scr = g.scratch ? g.scratch + (int64_t)blockIdx.x * g.lda : nullptr;
    const int tid = threadIdx.x;
    const int64_t plane = g.T * g.lda;
    const double2* zs2 = reinterpret_cast<const double2*>(g.zs);
    for (int64_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const int k = (int)(item % g.K);
        const int64_t t = g.dates[item / g.K];
        const int n = min(max(g.nrows[t], 0), (int)g.lda);
        const int64_t base = t * g.lda;
        const double* col = g.base + (int64_t)g.cols[k] * g.col_stride + base;
        const double2* zrow = Z ? zs2 + (int64_t)(g.zcols ? g.zcols[k] : k) * g.lda : nullptr;
        const int32_t* idx = g.rows_idx + base;
        double* out = g.ic + item * 3;
        // the column's value on row e < n (the asset index clamped to the plane)
        auto fval = [&](int e) {
            const int a = min(max(idx[e], 0), (int)g.lda - 1);
            double x = col[a];
            if constexpr (Z) {
                const double2 m = zrow[a];
                x = (x - m.x) * m.y;                       // as screen_ic_kernel
            }
            return x;
        };
        if (n == 0) {                                      // (uniform)
            if (tid < 3) out[tid] = qnan();
            continue;
        }
        int fin = 1;
        for (int e = tid; e < n; e += kRankThreads) fin &= __builtin_isfinite(fval(e));
        const bool col_fin = __syncthreads_and(fin);
        const i64 ry0 = g.rsum[t * 3], ry1 = g.rsum[t * 3 + 1], ry2 = g.rsum[t * 3 + 2];
        if (col_fin && ry0 >= 0 && ry1 >= 0 && ry2 >= 0) {
            // every value of the pair finite: one ranking over all n rows, mean = (n + 1) / 2
            sort_rows(lds, scr, n, [&](int e) { return okey(fval(e)); });
            const int32_t* rr = g.rrank + base;
            i64 sxx = 0, sxy0 = 0, sxy1 = 0, sxy2 = 0;
            for (int e = tid; e < n; e += kRankThreads) {
                const i64 dx = rank2(lds, scr, n, okey(fval(e))) - (n + 1);
                sxx += dx * dx;
                sxy0 += dx * (rr[e] - (n + 1));
                sxy1 += dx * (rr[plane + e] - (n + 1));
                sxy2 += dx * (rr[2 * plane + e] - (n + 1));
            }
            sxx = block_sum(sxx, sred);
            sxy0 = block_sum(sxy0, sred);
            sxy1 = block_sum(sxy1, sred);
            sxy2 = block_sum(sxy2, sred);
            if (tid == 0) {
                out[0] = spearman_finish(sxy0, sxx, ry0);
                out[1] = spearman_finish(sxy1, sxx, ry1);
                out[2] = spearman_finish(sxy2, sxx, ry2);
            }
            continue;
        }
        // the masked path, pair by pair
        for (int q = 0; q < 3; ++q) {
            const double* R = g.rows + (1 + q) * plane + base;
            i64 cm = 0, cne = 0;
            for (int e = tid; e < n; e += kRankThreads) {
                const bool fx = __builtin_isfinite(fval(e)), fy = __builtin_isfinite(R[e]);
                cm += fx && fy;
                cne += fx != fy;
            }
            const int nobs = (int)block_sum(cm, sred);
            // the masks agree on every row: the columns' own rankings (over their non-NaN rows,
            // +-inf included) stand; else both are ranked again over the common rows
            const bool own = block_sum(cne, sred) == 0;
            if (nobs == 0) {                               // (uniform)
                if (tid == 0) out[q] = qnan();
                continue;
            }
            sort_rows(lds, scr, n, [&](int e) {
                const double f = fval(e);
                const bool in = own ? f == f : __builtin_isfinite(f) && __builtin_isfinite(R[e]);
                return in ? okey(f) : kSortPad;
            });
            int rx[kRankPer];                              // 0: the row is not in the pair
#pragma unroll
            for (int j = 0; j < kRankPer; ++j) {
                const int e = j * kRankThreads + tid;
                rx[j] = 0;
                if (e < n) {
                    const double f = fval(e);
                    if (__builtin_isfinite(f) && __builtin_isfinite(R[e]))
                        rx[j] = rank2(lds, scr, n, okey(f));
                }
            }
            sort_rows(lds, scr, n, [&](int e) {
                const double r = R[e];
                const bool in = own ? r == r : __builtin_isfinite(r) && __builtin_isfinite(fval(e));
                return in ? okey(r) : kSortPad;
            });
            i64 sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int j = 0; j < kRankPer; ++j) {
                const int e = j * kRankThreads + tid;
                if (e < n && rx[j] != 0) {
                    const i64 dx = rx[j] - (nobs + 1);
                    const i64 dy = rank2(lds, scr, n, okey(R[e])) - (nobs + 1);
                    sxx += dx * dx;
                    syy += dy * dy;
                    sxy += dx * dy;
                }
            }
            sxx = block_sum(sxx, sred);
            syy = block_sum(syy, sred);
            sxy = block_sum(sxy, sred);
            if (tid == 0) out[q] = spearman_finish(sxy, sxx, syy);
        }
    }
}

bool rank_shape_ok(int64_t lda) { return lda > 0 && lda % 64 == 0 && lda <= kRankMaxRows; }

size_t rank_lds_bytes(int64_t lda) {
    return sizeof(u64) * (size_t)pow2_at_least((int)(lda < kRankLdsRows ? lda : kRankLdsRows));
}

}  // namespace
}  // namespace afm

using namespace afm;

extern "C" int64_t afm_rank_scratch_words(int64_t lda) {
    if (!rank_shape_ok(lda)) {
        afm_set_error("afm_rank_scratch_words: lda must be a positive multiple of 64 up to 32768");
        return -1;
    }
    return lda <= kRankLdsRows ? 0 : (int64_t)kRankSlots * lda;
}

extern "C" int afm_rank_returns_f64(afm_ctx* ctx, int64_t T, int64_t lda, const int32_t* dates,
                                    int64_t nd, const double* rows, const int32_t* nrows,
                                    int32_t* rrank, int64_t* rsum, uint64_t* scratch) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(T > 0 && rank_shape_ok(lda), "bad shape (lda a positive multiple of 64 up to 32768)");
    AFM_CHECK_ARG(dates && rows && nrows && rrank && rsum, "null buffer");
    AFM_CHECK_ARG(scratch || lda <= kRankLdsRows, "null buffer (scratch is needed past 16384 rows)");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(nd * 3 < (1ll << 31), "nd * 3 must be below 2^31");
    if (nd == 0) return AFM_OK;
    const int64_t items = nd * 3;
    const bool chunked = lda > kRankLdsRows;
    RankRetArgs g{T, lda, dates, items, rows, nrows, rrank, (i64*)rsum,
                  chunked ? (u64*)scratch : nullptr};
    const dim3 grid((unsigned)(chunked && items > kRankSlots ? kRankSlots : items));
    AFM_HIP(afm_lds_opt_in(ctx, (const void*)rank_returns_kernel, sizeof(u64) * kRankLdsRows));
    hipLaunchKernelGGL(rank_returns_kernel, grid, dim3(kRankThreads), rank_lds_bytes(lda),
                       ctx->stream, g);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_screen_rank_ic_f64(afm_ctx* ctx, const double* base, int64_t col_stride,
                                      int64_t T, int64_t lda, const int32_t* cols, int K,
                                      const double* zs, const int32_t* zcols,
                                      const int32_t* dates, int64_t nd, const double* rows,
                                      const int32_t* rows_idx, const int32_t* nrows,
                                      const int32_t* rrank, const int64_t* rsum,
                                      uint64_t* scratch, double* ic) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(T > 0 && rank_shape_ok(lda) && col_stride >= 0,
                  "bad shape (lda a positive multiple of 64 up to 32768)");
    AFM_CHECK_ARG(base && cols && dates && rows && rows_idx && nrows && rrank && rsum && ic,
                  "null buffer");
    AFM_CHECK_ARG(scratch || lda <= kRankLdsRows, "null buffer (scratch is needed past 16384 rows)");
    AFM_CHECK_ARG(zs || !zcols, "zcols without zs");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(nd * (int64_t)K < (1ll << 31), "nd * K must be below 2^31");
    if (nd == 0) return AFM_OK;
    const int64_t items = nd * K;
    const bool chunked = lda > kRankLdsRows;
    RankIcArgs g{base, col_stride, T, lda, cols, K, zs, zcols, dates, items, rows, rows_idx, nrows,
                 rrank, (const i64*)rsum, chunked ? (u64*)scratch : nullptr, ic};
    const dim3 grid((unsigned)(chunked && items > kRankSlots ? kRankSlots : items));
    const dim3 block(kRankThreads);
    const size_t lds = rank_lds_bytes(lda);
    if (zs) {
        AFM_HIP(afm_lds_opt_in(ctx, (const void*)rank_ic_kernel<true>, sizeof(u64) * kRankLdsRows));
        hipLaunchKernelGGL(rank_ic_kernel<true>, grid, block, lds, ctx->stream, g);
    } else {
        AFM_HIP(afm_lds_opt_in(ctx, (const void*)rank_ic_kernel<false>, sizeof(u64) * kRankLdsRows));
        hipLaunchKernelGGL(rank_ic_kernel<false>, grid, block, lds, ctx->stream, g);
    }
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
