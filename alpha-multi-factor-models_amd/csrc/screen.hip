// Factor screening (include/afm_screen.h): the per-date Pearson IC of K factor columns on one
// shared row set, the reference's one-column-at-a-time AlphaSignalAnalyzer(...).run() of KKT:465,
// 472 without the K-fold repetition -- forward returns, the merge / dropna cascade and the
// per-date demeans do not depend on the factor, so they are prepared once (analyzer.hip) and the
// panel is read once.
//
//  screen_ic_kernel       one wave per (date, 64 factor columns), lane = factor.  The date's rows
//                         go through LDS in chunks of kScreenRows: the loads run along the
//                         compacted rows of one plane (16 rows x 4 planes per instruction), the
//                         values -- z-scored on the way when zs is given -- are written
//                         transposed, and each lane walks its column in row order with the three
//                         nancorr recurrences (return_1 / 2 / 5) interleaved: xs_stats_kernel's
//                         `step` and finish, bit for bit.
//  screen_summary_kernel  one thread per (column, return, whole sample | year): n, mean, std,
//                         IR, t of the non-NaN ICs in numpy's summation order
//                         (xs_series_kernel's mean_over_std).
#include "afm_internal.h"
#include "afm_screen.h"

#pragma clang fp contract(off)

#include "afm_np_sum.h"

namespace afm {
namespace {

constexpr int kScreenLanes = 64;                   // factor columns per workgroup (one wave)
constexpr int kScreenRows = 16;                    // rows per staging chunk
constexpr int kScreenGroups = kScreenLanes / kScreenRows;   // planes per load instruction
constexpr int kScreenLoads = kScreenLanes / kScreenGroups;  // load instructions per chunk
// LDS row stride: lane-per-factor reads run along a row (consecutive doubles); the transposed
// writes run down the rows, 16 rows x 4 planes, and the odd stride spreads them over the banks
// (the zgram ring's padding)
constexpr int kScreenStride = kScreenLanes + 1;
constexpr int kScreenInv = 64;                     // 1 / (row number) ring: one divide per 64 rows
static_assert(kScreenInv % kScreenRows == 0 && kScreenInv == kScreenLanes, "ring refill");

struct ScreenArgs {
    const double* base;       // plane k: base + cols[k] * col_stride, [T][lda]
    int64_t col_stride, T, lda;
    const int32_t* cols;      // [K]
    int K;
    const double* zs;         // [..][lda][2] {mu, 1/sd}, or null: raw values
    const int32_t* zcols;     // [K] zs row of each column (null: row k)
    const int32_t* dates;     // [nd]
    int ngroups;              // ceil(K / kScreenLanes)
    const double* rows;       // [4][T][lda]: planes 1..3 the demeaned returns
    const int32_t* rows_idx;  // [T][lda]
    const int32_t* nrows;     // [T]
    double* ic;               // [nd][K][3]
};

template <bool Z>
__global__ __launch_bounds__(kScreenLanes) void screen_ic_kernel(ScreenArgs g) {
    __shared__ double sval[kScreenRows][kScreenStride];    // [row][factor lane]
    __shared__ double sret[3][kScreenRows];
    __shared__ double sinv[kScreenInv];
    __shared__ int64_t spoff[kScreenLanes];                // plane offset of each lane's column
    __shared__ int32_t szrow[kScreenLanes];                // its zs row
    const int lane = threadIdx.x;
    const int64_t di = blockIdx.x / g.ngroups;
    const int k0 = (int)(blockIdx.x % g.ngroups) * kScreenLanes;
    const int k = k0 + lane;
    const bool active = k < g.K;
    const int nk = min(kScreenLanes, g.K - k0);            // columns of this workgroup
    const int64_t t = g.dates[di];
    const int n = min(max(g.nrows[t], 0), (int)g.lda);
    const int64_t plane = g.T * g.lda, base = t * g.lda;
    spoff[lane] = active ? (int64_t)g.cols[k] * g.col_stride + base : 0;
    szrow[lane] = active ? (g.zcols ? g.zcols[k] : k) : 0;
    __syncthreads();
    // the loader's view of the wave: row r of the chunk, planes pg, pg + 4, ...
    const int r = lane % kScreenRows, pg = lane / kScreenRows;
    const double2* zs2 = reinterpret_cast<const double2*>(g.zs);
    double x[kScreenLoads], rv = 0.0;
    double2 m[Z ? kScreenLoads : 1];
    auto load_idx = [&](int c0) { return c0 + r < n ? g.rows_idx[base + c0 + r] : -1; };
    // Every load of a chunk is unconditional, so that all of them are issued back to back (a
    // tested load is a branch and a wait each): a lane without a row (a = -1) or without a column
    // reads a valid cell -- asset 0, the offset 0 of the unused lanes' spoff / szrow -- and its
    // value is dropped when the chunk is written to LDS
    auto load_chunk = [&](int c0, int a) {                 // a: the row's asset (-1: no row)
        const int ac = a < 0 ? 0 : a;
#pragma unroll
        for (int j = 0; j < kScreenLoads; ++j) {
            const int kk = kScreenGroups * j + pg;
            x[j] = g.base[spoff[kk] + ac];
            if constexpr (Z) m[j] = zs2[(int64_t)szrow[kk] * g.lda + ac];
        }
        const int64_t e = min((int64_t)c0 + r, g.lda - 1);
        rv = g.rows[(pg < 3 ? 1 + pg : 0) * plane + base + e];
    };
    int cnt[3] = {0, 0, 0};
    double mx[3] = {0, 0, 0}, my[3] = {0, 0, 0}, sxx[3] = {0, 0, 0}, syy[3] = {0, 0, 0},
           sxy[3] = {0, 0, 0};
    // the loads of a chunk are in flight while the previous chunk's recurrences run; the asset
    // indices they depend on are read one chunk further ahead
    int a_next = load_idx(0);
    load_chunk(0, a_next);
    a_next = load_idx(kScreenRows);
    for (int c0 = 0; c0 < n; c0 += kScreenRows) {
        const int len = min(kScreenRows, n - c0);
        __syncthreads();                                   // the previous chunk is consumed
        int fin = 1;
#pragma unroll
        for (int j = 0; j < kScreenLoads; ++j) {
            const int kk = kScreenGroups * j + pg;
            double v = x[j];
            if constexpr (Z) v = (v - m[j].x) * m[j].y;    // as the Gram and predict producers
            const bool ok = r < len && kk < nk;
            sval[r][kk] = ok ? v : 0.0;
            if (ok) fin &= __builtin_isfinite(v);
        }
        if (pg < 3) {
            sret[pg][r] = r < len ? rv : 0.0;
            if (r < len) fin &= __builtin_isfinite(rv);
        }
        if (c0 % kScreenInv == 0) sinv[lane] = 1. / (double)(c0 + lane + 1);
        const bool none_skipped = !active || (cnt[0] == c0 && cnt[1] == c0 && cnt[2] == c0);
        const bool fast = __syncthreads_and(fin && none_skipped);
        if (c0 + kScreenRows < n) {
            load_chunk(c0 + kScreenRows, a_next);
            a_next = load_idx(c0 + 2 * kScreenRows);
        }
        const double* iv = sinv + c0 % kScreenInv;
        if (fast) {
            // every value of the chunk finite and no lane has skipped a row: nobs == the row
            // number (1 / nobs from the table, no branch) and the three chains of a lane have
            // seen the same factor values, so they share the factor's mean and sum of squares
            double fm = my[0], fs = syy[0];
            auto step = [&](int e) {
                const double vy = sval[e][lane], inv = iv[e];
                const double dy = vy - fm;
                fm += inv * dy;
                fs += (vy - fm) * dy;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double vx = sret[q][e];
                    const double dx = vx - mx[q];
                    mx[q] += inv * dx;
                    sxx[q] += (vx - mx[q]) * dx;
                    sxy[q] += (vx - mx[q]) * dy;
                }
            };
            if (len == kScreenRows) {
#pragma unroll
                for (int e = 0; e < kScreenRows; ++e) step(e);
            } else {
                for (int e = 0; e < len; ++e) step(e);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                my[q] = fm;
                syy[q] = fs;
                cnt[q] += len;
            }
        } else {
            for (int e = 0; e < len; ++e) {
                const double vy = sval[e][lane];
                const bool fy = __builtin_isfinite(vy);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double vx = sret[q][e];
                    if (fy && __builtin_isfinite(vx)) {
                        cnt[q] += 1;
                        const double dx = vx - mx[q], dy = vy - my[q];
                        const double inv = cnt[q] == c0 + e + 1 ? iv[e] : 1. / (double)cnt[q];
                        mx[q] += inv * dx;
                        my[q] += inv * dy;
                        sxx[q] += (vx - mx[q]) * dx;
                        syy[q] += (vy - my[q]) * dy;
                        sxy[q] += (vx - mx[q]) * dy;
                    }
                }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double res = qnan();
        if (cnt[q] >= 1) {
            const double div = __builtin_sqrt(sxx[q] * syy[q]);
            if (div != 0) res = sxy[q] / div;
        }
        g.ic[(di * g.K + k) * 3 + q] = res;
    }
}

// ---- summary: whole-sample statistics and the per-year IR of every (column, return) ----------
// Task (kq, part): part 0 = the whole sample, part 1 + y = year year0 + y.  The task's non-NaN
// ICs are collected in date order into its own run of the scratch -- the whole-sample row
// [kq][0][nd], or inside the years' row [kq][1][nd] at the number of dates of earlier years (the
// years' runs do not overlap, whatever the order of the dates) -- and summed as pandas does.
__global__ __launch_bounds__(64) void screen_summary_kernel(const double* ic, int64_t nd, int K,
                                                            const int32_t* year, int nyears,
                                                            int year0, double* stats,
                                                            double* ir_year, double* scratch) {
    const int64_t K3 = (int64_t)K * 3;
    const int64_t task = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (task >= K3 * (nyears + 1)) return;
    const int64_t kq = task % K3;
    const int part = (int)(task / K3);
    const int yr = year0 + part - 1;
    double* buf = scratch + (kq * 2 + (part ? 1 : 0)) * nd;
    if (part) {
        int64_t before = 0;
        for (int64_t i = 0; i < nd; ++i) before += year[i] < yr;
        buf += before;
    }
    int64_t n = 0;
    for (int64_t i = 0; i < nd; ++i) {
        const double v = ic[i * K3 + kq];
        if ((!part || year[i] == yr) && v == v) buf[n++] = v;
    }
    double mean = qnan(), sd = qnan();                     // xs_series_kernel's mean_over_std
    if (n > 0) {
        mean = seq_np_sum(buf, n) / (double)n;
        if (n > 1) {
            const double avg = seq_np_sum(buf, n) / (double)n;
            for (int64_t i = 0; i < n; ++i) {
                const double d = avg - buf[i];
                buf[i] = d * d;
            }
            sd = __builtin_sqrt(seq_np_sum(buf, n) / ((double)n - 1.0));
        }
    }
    const double ir = n > 0 ? mean / sd : qnan();
    if (part) {
        ir_year[(int64_t)(part - 1) * K3 + kq] = ir;
    } else {
        double* s = stats + kq * 5;
        s[0] = (double)n;
        s[1] = mean;
        s[2] = sd;
        s[3] = ir;
        s[4] = ir * __builtin_sqrt((double)n);
    }
}

}  // namespace
}  // namespace afm

using namespace afm;

extern "C" int afm_screen_ic_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                                 int64_t lda, const int32_t* cols, int K, const double* zs,
                                 const int32_t* zcols, const int32_t* dates, int64_t nd,
                                 const double* rows, const int32_t* rows_idx,
                                 const int32_t* nrows, double* ic) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(T > 0 && lda > 0 && lda % 64 == 0 && col_stride >= 0,
                  "bad shape (lda a positive multiple of 64)");
    AFM_CHECK_ARG(base && cols && dates && rows && rows_idx && nrows && ic, "null buffer");
    AFM_CHECK_ARG(zs || !zcols, "zcols without zs");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    const int64_t ngroups = ((int64_t)K + kScreenLanes - 1) / kScreenLanes;
    AFM_CHECK_ARG(nd * ngroups < (1ll << 31), "nd * ceil(K / 64) must be below 2^31");
    if (nd == 0) return AFM_OK;
    ScreenArgs g{base, col_stride, T, lda, cols, K, zs, zcols, dates, (int)ngroups, rows, rows_idx,
                 nrows, ic};
    const dim3 grid((unsigned)(nd * ngroups)), block(kScreenLanes);
    if (zs) hipLaunchKernelGGL(screen_ic_kernel<true>, grid, block, 0, ctx->stream, g);
    else hipLaunchKernelGGL(screen_ic_kernel<false>, grid, block, 0, ctx->stream, g);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_screen_summary_f64(afm_ctx* ctx, const double* ic, int64_t nd, int K,
                                      const int32_t* year, int nyears, int year0, double* stats,
                                      double* ir_year, double* scratch) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(nyears >= 0 && nyears <= 320, "nyears must be in [0, 320]");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(ic && year && stats && ir_year && scratch, "null buffer");
    const int64_t tasks = (int64_t)K * 3 * (nyears + 1);
    hipLaunchKernelGGL(screen_summary_kernel, dim3((unsigned)((tasks + 63) / 64)), dim3(64), 0,
                       ctx->stream, ic, nd, K, year, nyears, year0, stats, ir_year, scratch);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
