// Factor combination (include/afm_combine.h): the rolling IC weights of the screened columns and
// the weighted composite plane.
//
// afm_ic_weights_f64 -- one workgroup per position i.
//   Methods 0..2 (icw_roll_kernel, 128 threads): thread k walks the window of column k in
//   ascending j -- ic[j][k][q], stride 3 doubles across the lanes, the rows L2-resident -- once
//   for the mean and once for the squares; thread 0 normalises in ascending k.  One add per term,
//   no FMA (the build has -ffp-contract=off): a numpy loop gives the same bits.
//   Method 3 (icw_maxir_kernel, 256 threads): the candidates' counts, the complete dates D
//   compacted into an LDS list, the means and variances over D per column, then the centred Gram
//   of the active columns streamed through LDS in chunks of kIcwChunk dates -- every thread keeps
//   the lower-triangle part of an 8 x 8 tile of the 128 x 128 matrix in registers (36 VALU FMAs
//   per date) --, the shrunk matrix in LDS
//   ((K + 1)-strided rows, up to 129 KB: the opt-in of portfolio.hip), a right-looking Cholesky
//   and two column-oriented triangular solves, all in the workgroup.  Every order is fixed by the
//   window's own contents: a row is a function of its window alone.
//
// afm_combine_f64 -- the hot path: one lane per row of a date, 256 rows per workgroup, grid
//   (nd, ceil(lda / 256)).  Wave 0 compacts the date's weights (finite, not 0) with their plane
//   offsets into LDS, so a column without weight is never read; the k loop is unrolled by
//   kCbUnroll with all loads of a batch issued before the first multiply-add (the order of the
//   arithmetic is ascending k).  The workgroup of asset block b also writes NaN / 0 into the
//   cells of [256 b, 256 b + 256) that are on no row of the date: it marks the block's assets
//   from the date's rows_idx (plain byte stores into LDS), so result cells and filler cells are
//   disjoint and no order between workgroups is needed.  No atomics, no scratch.
#include "afm_internal.h"
#include "afm_combine.h"

#include <cmath>
#include <vector>

namespace afm {
namespace {

constexpr int kMaxK = AFM_COMBINE_MAX_K;
constexpr int kMaxWin = AFM_COMBINE_MAX_WINDOW;
constexpr int kRollThreads = 128;
constexpr int kMxThreads = 256;
constexpr int kIcwChunk = 16;          // dates per LDS chunk of the Gram
constexpr int kCbThreads = 256;
constexpr int kCbUnroll = 8;

__device__ __forceinline__ double cb_nan() { return __builtin_nan(""); }

struct IcwArgs {
    const double* ic;
    int64_t nd;
    int K, q, method, window, embargo, minp;
    double shrink;
    double* w;
    double* info;
};

// thread 0: w row and info from the raw values of the active columns, ascending k
__device__ __forceinline__ double icw_total(const double* raw, const uint8_t* act, int K,
                                            int* n_active) {
    double sum = 0.0;
    int na = 0;
    for (int k = 0; k < K; ++k)
        if (act[k]) {
            sum += fabs(raw[k]);
            ++na;
        }
    *n_active = na;
    return sum;
}

__global__ __launch_bounds__(kRollThreads) void icw_roll_kernel(IcwArgs g) {
    __shared__ double sraw[kMaxK];
    __shared__ int sn[kMaxK];
    __shared__ uint8_t sact[kMaxK];
    __shared__ double ssum;
    __shared__ int sok;
    const int k = threadIdx.x, K = g.K;
    const int64_t i = blockIdx.x;
    const int64_t j1 = i - g.embargo;                      // < 0: the window is empty
    const int64_t j0 = j1 - g.window + 1 > 0 ? j1 - g.window + 1 : 0;
    double raw = 0.0;
    bool act = false;
    int n = 0;
    if (k < K) {
        if (g.method == AFM_COMBINE_EQUAL) {
            raw = 1.0;
            act = true;
        } else {
            const int64_t step = (int64_t)K * 3;
            const double* p = g.ic + (j0 * K + k) * 3 + g.q;
            double s = 0.0;
            for (int64_t j = j0; j <= j1; ++j) {
                const double v = p[(j - j0) * step];
                if (__builtin_isfinite(v)) {
                    s += v;
                    ++n;
                }
            }
            if (n >= g.minp) {
                const double m = s / (double)n;
                if (g.method == AFM_COMBINE_IC) {
                    raw = m;
                    act = true;
                } else {
                    double ss = 0.0;
                    for (int64_t j = j0; j <= j1; ++j) {
                        const double v = p[(j - j0) * step];
                        if (__builtin_isfinite(v)) {
                            const double d = v - m;
                            ss += d * d;
                        }
                    }
                    const double sd = sqrt(ss / (double)(n - 1));
                    act = __builtin_isfinite(sd) && sd > 0.0;
                    raw = act ? m / sd : 0.0;
                }
            }
        }
        sraw[k] = raw;
        sact[k] = act;
        sn[k] = n;
    }
    __syncthreads();
    if (k == 0) {
        int na, nmax = 0;
        const double sum = icw_total(sraw, sact, K, &na);
        for (int c = 0; c < K; ++c) nmax = sn[c] > nmax ? sn[c] : nmax;
        const bool ok = na > 0 && __builtin_isfinite(sum) && sum > 0.0;
        ssum = sum;
        sok = ok;
        double* info = g.info + i * 3;
        info[0] = (double)na;
        info[1] = (double)nmax;
        info[2] = sum;
    }
    __syncthreads();
    if (k < K) g.w[i * K + k] = sok ? (act ? raw / ssum : 0.0) : cb_nan();
}

// wave 0: the indices e < n with flag[e] set, ascending, into list; returns their number (to
// every lane of wave 0)
template <typename L>
__device__ __forceinline__ int compact_flags(const uint8_t* flag, int n, L* list, int lane) {
    int cnt = 0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        const bool on = e < n && flag[e];
        const unsigned long long m = __ballot(on);
        if (on) list[cnt + __popcll(m & ((1ull << lane) - 1ull))] = (L)e;
        cnt += __popcll(m);
    }
    return cnt;
}

struct MxShared {
    double mean[kMaxK];                // by active slot
    double rhs[kMaxK];
    double y[kMaxK];
    double x[kMaxK];
    double piv[kMaxK];                 // sqrt of the pivots
    double raw[kMaxK];                 // by column
    double chunk[kIcwChunk * kMaxK];
    int16_t dlist[kMaxWin];
    int16_t alist[kMaxK];
    uint8_t dflag[kMaxWin];
    uint8_t cand[kMaxK];
    uint8_t act[kMaxK];
    int nD, na, ok;
    double sum;
};

__global__ __launch_bounds__(kMxThreads) void icw_maxir_kernel(IcwArgs g) {
    extern __shared__ __attribute__((aligned(16))) double Am[];      // [K][K + 1]
    __shared__ MxShared sh;
    const int tid = threadIdx.x, lane = tid & 63, K = g.K, q = g.q;
    const int LD = K + 1;
    const int64_t i = blockIdx.x;
    const int64_t j1 = i - g.embargo;
    const int64_t j0 = j1 - g.window + 1 > 0 ? j1 - g.window + 1 : 0;
    const int L = j1 >= j0 ? (int)(j1 - j0 + 1) : 0;       // dates of the window
    const int64_t step = (int64_t)K * 3;
    const double* win = g.ic + j0 * step + q;              // date e, column k: [e * step + 3 k]
    // ---- 1. candidates -------------------------------------------------------------------------
    for (int e = tid; e < L; e += kMxThreads) sh.dflag[e] = 1;
    if (tid < K) {
        int n = 0;
        for (int e = 0; e < L; ++e) n += __builtin_isfinite(win[e * step + 3 * tid]) ? 1 : 0;
        sh.cand[tid] = n >= g.minp;
        sh.act[tid] = 0;
        sh.raw[tid] = 0.0;
    }
    __syncthreads();
    // ---- 2. D: the dates on which every candidate is finite ------------------------------------
    if (tid < K && sh.cand[tid])
        for (int e = 0; e < L; ++e)
            if (!__builtin_isfinite(win[e * step + 3 * tid])) sh.dflag[e] = 0;
    __syncthreads();
    if (tid < 64) {
        const int c = compact_flags(sh.dflag, L, sh.dlist, lane);
        if (tid == 0) sh.nD = c;
    }
    __syncthreads();
    const int nD = sh.nD;
    const bool enough = nD >= g.minp;
    // ---- 3. means and variances over D; the active columns -------------------------------------
    double mk = 0.0;
    if (enough && tid < K && sh.cand[tid]) {
        // the mean by a compensated sum (two_sum per term): a mean that nearly cancels stays good
        // to its own ulp, which the backward error of the solve is measured against
        double s = 0.0, tail = 0.0;
        for (int d = 0; d < nD; ++d) {
            const double v = win[sh.dlist[d] * step + 3 * tid];
            const double t = s + v, bp = t - s;
            tail += (s - (t - bp)) + (v - bp);
            s = t;
        }
        mk = (s + tail) / (double)nD;
        double ss = 0.0;
        for (int d = 0; d < nD; ++d) {
            const double c = win[sh.dlist[d] * step + 3 * tid] - mk;
            ss += c * c;
        }
        sh.act[tid] = ss / (double)(nD - 1) > 0.0;
    }
    __syncthreads();
    if (tid < 64) {
        const int c = compact_flags(sh.act, K, sh.alist, lane);
        if (tid == 0) sh.na = c;
    }
    __syncthreads();
    const int na = sh.na;
    if (tid < K && sh.act[tid]) {                          // the slot of column tid
        int s = 0;
        for (int c = 0; c < tid; ++c) s += sh.act[c];
        sh.mean[s] = mk;
        sh.rhs[s] = mk;
    }
    __syncthreads();
    bool fail = false;
    if (na > 0) {
        // ---- 4. the centred Gram of the active columns: 8 x 8 register tiles -------------------
        const int ty = tid >> 4, tx = tid & 15;            // slots ty + 16 u, tx + 16 v
        double acc[8][8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int v = 0; v < 8; ++v) acc[u][v] = 0.0;
        for (int d0 = 0; d0 < nD; d0 += kIcwChunk) {
            const int cn = nD - d0 < kIcwChunk ? nD - d0 : kIcwChunk;
            __syncthreads();
            for (int idx = tid; idx < kIcwChunk * kMaxK; idx += kMxThreads) {
                const int d = idx >> 7, a = idx & (kMaxK - 1);
                double c = 0.0;
                if (d < cn && a < na)
                    c = win[sh.dlist[d0 + d] * step + 3 * sh.alist[a]] - sh.mean[a];
                sh.chunk[idx] = c;
            }
            __syncthreads();
            for (int d = 0; d < cn; ++d) {
                const double* row = sh.chunk + d * kMaxK;
                double ca[8], cb[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    ca[u] = row[ty + 16 * u];
                    cb[u] = row[tx + 16 * u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (16 * u < na) {                     // (uniform)
#pragma unroll
                        for (int v = 0; v <= u; ++v)       // the lower triangle's tiles only
                            acc[u][v] = __builtin_fma(ca[u], cb[v], acc[u][v]);
                    }
                }
            }
        }
        const double off = 1.0 - g.shrink, denom = (double)(nD - 1);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int v = 0; v <= u; ++v) {
                const int a = ty + 16 * u, b = tx + 16 * v;
                if (a < na && b <= a) {                    // (the Cholesky reads b <= a only)
                    const double s = acc[u][v] / denom;
                    Am[a * LD + b] = a == b ? off * s + g.shrink * s : off * s;
                }
            }
        // ---- 5. Cholesky (lower), right-looking ------------------------------------------------
        for (int p = 0; p < na; ++p) {
            __syncthreads();
            const double d = Am[p * LD + p];
            if (!(d > 0.0)) {                              // (uniform: every thread reads the cell)
                fail = true;
                break;
            }
            const double l = sqrt(d);
            if (tid == 0) sh.piv[p] = l;
            for (int r = p + 1 + tid; r < na; r += kMxThreads) Am[r * LD + p] /= l;
            __syncthreads();
            const int m = na - p - 1;
            for (int r0 = ty; r0 < m; r0 += 16) {
                const int r = p + 1 + r0;
                const double lr = Am[r * LD + p];
                for (int c0 = tx; c0 <= r0; c0 += 16) {
                    const int c = p + 1 + c0;
                    Am[r * LD + c] = __builtin_fma(-lr, Am[c * LD + p], Am[r * LD + c]);
                }
            }
        }
        // ---- 6. L y = m, L' x = y ---------------------------------------------------------------
        if (!fail) {
            for (int p = 0; p < na; ++p) {
                __syncthreads();
                const double y = sh.rhs[p] / sh.piv[p];
                if (tid == 0) sh.y[p] = y;
                for (int r = p + 1 + tid; r < na; r += kMxThreads)
                    sh.rhs[r] = __builtin_fma(-Am[r * LD + p], y, sh.rhs[r]);
            }
            for (int p = na - 1; p >= 0; --p) {
                __syncthreads();
                const double x = sh.y[p] / sh.piv[p];
                if (tid == 0) sh.x[p] = x;
                for (int r = tid; r < p; r += kMxThreads)
                    sh.y[r] = __builtin_fma(-Am[p * LD + r], x, sh.y[r]);
            }
            __syncthreads();
            if (tid < na) sh.raw[sh.alist[tid]] = sh.x[tid];
        }
    }
    __syncthreads();
    if (tid == 0) {
        int cnt;
        double sum = icw_total(sh.raw, sh.act, K, &cnt);
        if (fail) sum = cb_nan();
        sh.ok = cnt > 0 && __builtin_isfinite(sum) && sum > 0.0;
        sh.sum = sum;
        double* info = g.info + i * 3;
        info[0] = (double)cnt;
        info[1] = (double)nD;
        info[2] = sum;
    }
    __syncthreads();
    if (tid < K) g.w[i * K + tid] = sh.ok ? (sh.act[tid] ? sh.raw[tid] / sh.sum : 0.0) : cb_nan();
}

struct CbArgs {
    const double* base;
    int64_t col_stride, T, lda;
    const int32_t* cols;
    int K;
    const double* zs;
    const int32_t* zcols;
    const int32_t* dates;
    const int32_t* rows_idx;
    const int32_t* nrows;
    const double* w;
    int64_t w_stride;
    double* out;
    int32_t* cnt;
};

template <bool Z>
__global__ __launch_bounds__(kCbThreads) void combine_kernel(CbArgs g) {
    __shared__ double sw[kMaxK];                           // the date's weights that count,
    __shared__ int64_t soff[kMaxK];                        // the offsets of their planes
    __shared__ int64_t szo[Z ? kMaxK : 1];                 // and of their rows of zs (double2)
    __shared__ int sna;
    __shared__ uint8_t sflag[kCbThreads];                  // asset of this block is on a row
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t di = blockIdx.x;
    const int64_t t = g.dates[di];
    if (t < 0 || t >= g.T) return;
    const int64_t lda = g.lda, rowbase = t * lda;
    const int64_t a0 = (int64_t)blockIdx.y * kCbThreads;
    int64_t n_rows = g.nrows[t];
    n_rows = n_rows < 0 ? 0 : (n_rows > lda ? lda : n_rows);
    sflag[tid] = 0;
    if (tid < 64) {
        const double* wrow = g.w + di * g.w_stride;
        int cnt = 0;
        for (int k0 = 0; k0 < g.K; k0 += 64) {
            const int k = k0 + lane;
            const double wk = k < g.K ? wrow[k] : 0.0;
            const bool on = k < g.K && __builtin_isfinite(wk) && wk != 0.0;
            const unsigned long long m = __ballot(on);
            if (on) {
                const int s = cnt + __popcll(m & ((1ull << lane) - 1ull));
                sw[s] = wk;
                soff[s] = (int64_t)g.cols[k] * g.col_stride;
                if constexpr (Z) szo[s] = (int64_t)(g.zcols ? g.zcols[k] : k) * lda;
            }
            cnt += __popcll(m);
        }
        if (tid == 0) sna = cnt;
    }
    __syncthreads();
    for (int64_t e = tid; e < n_rows; e += kCbThreads) {
        const int64_t a = (int64_t)g.rows_idx[rowbase + e] - a0;
        if (a >= 0 && a < kCbThreads && a + a0 < lda) sflag[a] = 1;
    }
    const int na = sna;
    const int64_t e = a0 + tid;
    if (e < n_rows) {
        const int64_t a = g.rows_idx[rowbase + e];
        if (a >= 0 && a < lda) {
            const double* cell = g.base + rowbase + a;
            const double2* zs2 = Z ? reinterpret_cast<const double2*>(g.zs) + a : nullptr;
            double num = 0.0, den = 0.0;
            int c = 0;
            for (int k0 = 0; k0 < na; k0 += kCbUnroll) {
                double x[kCbUnroll];
                double2 mz[Z ? kCbUnroll : 1];
#pragma unroll
                for (int u = 0; u < kCbUnroll; ++u) {
                    const int s = k0 + u < na ? k0 + u : na - 1;
                    x[u] = cell[soff[s]];
                    if constexpr (Z) mz[u] = zs2[szo[s]];
                }
#pragma unroll
                for (int u = 0; u < kCbUnroll; ++u) {
                    double v = x[u];
                    if constexpr (Z) v = (v - mz[u].x) * mz[u].y;  // as the IC kernel reads it
                    if (k0 + u < na && __builtin_isfinite(v)) {
                        const double wk = sw[k0 + u];
                        const double pr = wk * v;
                        num += pr;
                        den += fabs(wk);
                        ++c;
                    }
                }
            }
            g.out[rowbase + a] = c ? num / den : cb_nan();
            if (g.cnt) g.cnt[rowbase + a] = c;
        }
    }
    __syncthreads();
    if (e < lda && !sflag[tid]) {
        g.out[rowbase + e] = cb_nan();
        if (g.cnt) g.cnt[rowbase + e] = 0;
    }
}

}  // namespace
}  // namespace afm

using namespace afm;

extern "C" int afm_ic_weights_f64(afm_ctx* ctx, const double* ic, int64_t nd, int K, int q,
                                  int method, int window, int embargo, int min_periods,
                                  double shrink, double* w, double* info) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1 && K <= kMaxK, "K must be in 1..128");
    AFM_CHECK_ARG(window >= 1 && window <= kMaxWin, "window must be in 1..1024");
    AFM_CHECK_ARG(embargo >= 0, "embargo is negative");
    AFM_CHECK_ARG(method >= AFM_COMBINE_EQUAL && method <= AFM_COMBINE_MAXIR, "unknown method");
    AFM_CHECK_ARG(min_periods >= 1 && min_periods <= window, "min_periods must be in 1..window");
    if (method >= AFM_COMBINE_ICIR)
        AFM_CHECK_ARG(min_periods >= 2, "min_periods must be at least 2 for this method");
    AFM_CHECK_ARG(q >= 0 && q <= 2, "q must be in 0..2");
    if (method == AFM_COMBINE_MAXIR)
        AFM_CHECK_ARG(shrink > 0.0 && shrink <= 1.0, "shrink must be in (0, 1]");
    AFM_CHECK_ARG(nd >= 0 && nd < (1ll << 31), "nd must be in 0..2^31 - 1");
    if (nd == 0) return AFM_OK;
    AFM_CHECK_ARG(ic && w && info, "null buffer");
    IcwArgs g{ic, nd, K, q, method, window, embargo, min_periods, shrink, w, info};
    if (method == AFM_COMBINE_MAXIR) {
        const size_t smem = sizeof(double) * (size_t)K * (size_t)(K + 1);
        AFM_HIP(afm_lds_opt_in(ctx, (const void*)icw_maxir_kernel, (int)smem));
        hipLaunchKernelGGL(icw_maxir_kernel, dim3((unsigned)nd), dim3(kMxThreads), smem,
                           ctx->stream, g);
    } else {
        hipLaunchKernelGGL(icw_roll_kernel, dim3((unsigned)nd), dim3(kRollThreads), 0, ctx->stream,
                           g);
    }
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_combine_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                               int64_t lda, const int32_t* cols, int K, const double* zs,
                               const int32_t* zcols, const int32_t* dates, int64_t nd,
                               const int32_t* rows_idx, const int32_t* nrows, const double* w,
                               int64_t w_stride, double* out, int32_t* cnt) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1 && K <= kMaxK, "K must be in 1..128");
    AFM_CHECK_ARG(T > 0 && lda > 0 && lda % 64 == 0 && col_stride >= 0,
                  "bad shape (lda a positive multiple of 64)");
    AFM_CHECK_ARG(w_stride == 0 || w_stride == K, "w_stride must be 0 or K");
    AFM_CHECK_ARG(zs || !zcols, "zcols without zs");
    AFM_CHECK_ARG(nd >= 0 && nd < (1ll << 31), "nd must be in 0..2^31 - 1");
    AFM_CHECK_ARG(lda <= (int64_t)kCbThreads * 65535, "lda is too large");
    if (nd == 0) return AFM_OK;
    AFM_CHECK_ARG(base && cols && dates && rows_idx && nrows && w && out, "null buffer");
    {   // out against the planes the call reads (cols comes to the host for it)
        std::vector<int32_t> hc((size_t)K);
        AFM_HIP(hipMemcpyAsync(hc.data(), cols, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost,
                               ctx->stream));
        AFM_HIP(hipStreamSynchronize(ctx->stream));
        const int64_t plane = T * lda;
        for (int k = 0; k < K; ++k) {
            AFM_CHECK_ARG(hc[(size_t)k] >= 0, "negative column");
            const double* p0 = base + (int64_t)hc[(size_t)k] * col_stride;
            AFM_CHECK_ARG(p0 + plane <= out || out + plane <= p0, "out overlaps a plane it reads");
        }
    }
    CbArgs g{base, col_stride, T, lda, cols, K, zs, zcols, dates, rows_idx, nrows, w, w_stride,
             out, cnt};
    const dim3 grid((unsigned)nd, (unsigned)((lda + kCbThreads - 1) / kCbThreads));
    if (zs)
        hipLaunchKernelGGL(combine_kernel<true>, grid, dim3(kCbThreads), 0, ctx->stream, g);
    else
        hipLaunchKernelGGL(combine_kernel<false>, grid, dim3(kCbThreads), 0, ctx->stream, g);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
