// Cross-factor correlation of the factor screen (include/afm_xcorr.h): per evaluated date the
// pairwise-complete Pearson correlation matrix of the K screened columns on the screen's shared
// rows -- pandas DataFrame.corr() -- as masked Grams on v_mfma_f64_16x16x4_f64, and its summary
// over the dates.
//
//  xcorr_kernel          one workgroup (4 waves) per (date, pair of 64-column blocks BI <= BJ); wave
//                        w owns tile row w of the 64 x 64 block: 4 accumulator tiles of 16 x 16.
//                        Three passes over the date's rows, staged 32 at a time through an LDS tile
//                        [column][row] (row stride 34: the Gram kernels' padding, 4 banks a column):
//                          1. each column's first finite value c0 (one thread per column);
//                          2. its row count, mean and sd of v - c0 over its own finite rows (two
//                             threads per column, fixed order);
//                          3. the products of U = ((v - c0) - mean) / sd, 0 where missing, and the
//                             presence M: N = M'M, P = U'U, S = U'M, Q = (U.U)'M.
//                        A workgroup whose columns have no missing cell forms only P and the column
//                        sums (U'1, (U.U)'1, one MFMA per tile row / column instead of one per
//                        tile): the same MFMA shape and the same operands as the masked products
//                        take with an all-ones M, so both paths give the same bits.  The shift and
//                        scale of a column depend on that column alone, so an entry depends on its
//                        two columns alone.  Upper triangle computed, mirrored on the way out.
//                        The masked path takes the tile columns two at a time (12 accumulator
//                        tiles a wave): two workgroups fit a CU.
//  xcorr_summary_kernel  one thread per pair: n, mean r, mean |r| over the dates in numpy's
//                        summation order.
// Algorithmic work per date: rows * K (K + 1) flops on the fast path (the symmetric product),
// six times that on the masked one; rows * K * 8 B read three times (L2 after the first).
#include "afm_internal.h"
#include "afm_xcorr.h"

#pragma clang fp contract(off)

#include "afm_np_sum.h"

namespace afm {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kXcBlock = 64;                  // columns per block (4 tiles of 16)
constexpr int kXcTiles = kXcBlock / 16;
constexpr int kXcCols = 2 * kXcBlock;         // staged columns: block BI, then block BJ
constexpr int kXcRows = 32;                   // rows per staging chunk
constexpr int kXcRS = kXcRows + 2;                     // LDS tile row stride (doubles)
constexpr int kXcThreads = 256;
constexpr int kXcGroups = kXcThreads / kXcRows;   // column groups of the staging threads
constexpr int kXcBatch = 8;                   // loads in flight per thread while staging
static_assert(kXcThreads == 2 * kXcCols && kXcRows % 4 == 0, "thread maps");
static_assert(kXcBlock % (kXcGroups * kXcBatch) == 0, "staging batches");
static_assert(kXcThreads / 64 == kXcTiles, "one wave per tile row");

struct XcorrArgs {
    const double* base;       // plane k: base + cols[k] * col_stride, [T][lda]
    int64_t col_stride, T, lda;
    const int32_t* cols;      // [K]
    int K;
    const double* zs;         // [..][lda][2] {mu, 1/sd}, or null: raw values
    const int32_t* zcols;     // [K] zs row of each column (null: row k)
    const int32_t* dates;     // [nd]
    int nblocks, npairs;      // ceil(K / 64), nblocks (nblocks + 1) / 2
    const int32_t* rows_idx;  // [T][lda]
    const int32_t* nrows;     // [T]
    double* xc;               // [nd][K][K]
};

struct XcorrSmem {
    double tile[kXcCols][kXcRS];              // [column][row of the chunk]
    int64_t poff[kXcCols];                    // plane offset of the column at the date
    int32_t zrow[kXcCols];                    // its zs row
    int32_t colid[kXcCols];                   // its cols[] entry (-1: no column)
    double c0[kXcCols], mean[kXcCols], scale[kXcCols];
    double ps1[kXcThreads], ps2[kXcThreads], pmin[kXcThreads], pmax[kXcThreads];
    int pcnt[kXcThreads];
    double sb[kXcBlock], qb[kXcBlock];        // fast path: column sums of block BJ
};

// the correlation of one pair from its moments over the joint rows; symmetric in (a, b) bit for
// bit (every product commutes)
__device__ __forceinline__ double xcorr_entry(const double N, const double P, const double Sa,
                                              const double Sb, const double Qa, const double Qb,
                                              const bool same) {
    if (!(N >= 2.0)) return qnan();
    const double va = Qa - Sa * Sa / N, vb = Qb - Sb * Sb / N;
    if (!(va > 0.0) || !(vb > 0.0)) return qnan();
    if (same) return 1.0;
    const double r = (P - Sa * Sb / N) / __builtin_sqrt(va * vb);
    return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
}

template <bool Z>
__global__ __launch_bounds__(kXcThreads) void xcorr_kernel(XcorrArgs g) {
    __shared__ XcorrSmem sm;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t di = blockIdx.x / g.npairs;
    int bi = 0, bj = 0;
    {                                                      // pair index -> (bi <= bj), row-major
        int q = (int)(blockIdx.x % g.npairs);
        while (q >= g.nblocks - bi) { q -= g.nblocks - bi; ++bi; }
        bj = bi + q;
    }
    const bool diag = bi == bj;
    const int ncol = diag ? kXcBlock : kXcCols;            // staged columns
    const int jbase = diag ? 0 : kXcBlock;                 // tile columns of block BJ
    const int64_t t = g.dates[di];
    const int n = min(max(g.nrows[t], 0), (int)g.lda);
    const int64_t base = t * g.lda;
    const double2* zs2 = reinterpret_cast<const double2*>(g.zs);
    if (tid < kXcCols) {
        const int k = (tid < kXcBlock ? bi * kXcBlock : bj * kXcBlock - kXcBlock) + tid;
        const bool have = tid < ncol && k < g.K;
        const int col = have ? g.cols[k] : -1;
        sm.colid[tid] = col;
        sm.poff[tid] = have ? (int64_t)col * g.col_stride + base : base;
        sm.zrow[tid] = have ? (g.zcols ? g.zcols[k] : k) : 0;
    }
    __syncthreads();
    // the value of column c at asset a: the double afm_screen_ic_f64 reads
    auto value = [&](int c, int a) {
        double v = g.base[sm.poff[c] + a];
        if constexpr (Z) {
            const double2 m = zs2[(int64_t)sm.zrow[c] * g.lda + a];
            v = (v - m.x) * m.y;
        }
        return v;
    };
    auto asset = [&](int e) { return min(max(g.rows_idx[base + e], 0), (int)g.lda - 1); };

    // ---- pass 1: the first finite value of every column -----------------------------------------
    if (tid < kXcCols) {
        double c0 = 0.0;
        if (sm.colid[tid] >= 0) {
            for (int e = 0; e < n; ++e) {
                const double v = value(tid, asset(e));
                if (__builtin_isfinite(v)) { c0 = v; break; }
            }
        }
        sm.c0[tid] = c0;
    }
    __syncthreads();

    // Staging of the chunk at row r0: thread (row sr, column group sg), columns sg, sg + 8, ...
    // -- the loads of a half-wave run along the compacted rows of one plane.
    // put(c, r, present, d): d = v - c0 of the cell, present: the row and the column exist.
    const int sr = tid % kXcRows, sg = tid / kXcRows;
    auto stage = [&](int r0, auto put) {
        const bool rowok = r0 + sr < n;
        const int a = rowok ? asset(r0 + sr) : 0;
        for (int j0 = 0; j0 < ncol / kXcGroups; j0 += kXcBatch) {
            double v[kXcBatch];
#pragma unroll
            for (int j = 0; j < kXcBatch; ++j) v[j] = value(sg + kXcGroups * (j0 + j), a);
#pragma unroll
            for (int j = 0; j < kXcBatch; ++j) {
                const int c = sg + kXcGroups * (j0 + j);
                put(c, sr, rowok && sm.colid[c] >= 0, v[j] - sm.c0[c]);
            }
        }
    };

    // ---- pass 2: count, mean and sd of d = v - c0 over the column's present rows ----------------
    {
        const int c = tid >> 1, h = tid & 1;               // column, half of the chunk's rows
        double s1 = 0.0, s2 = 0.0, dmin = 0.0, dmax = 0.0;
        int cnt = 0;
        for (int r0 = 0; r0 < n; r0 += kXcRows) {
            __syncthreads();
            stage(r0, [&](int cc, int r, bool present, double d) {
                sm.tile[cc][r] = present ? d : qnan();
            });
            __syncthreads();
            if (c < ncol) {
                for (int e = 0; e < kXcRows / 2; ++e) {
                    const double d = sm.tile[c][h * (kXcRows / 2) + e];
                    if (__builtin_isfinite(d)) {
                        dmin = cnt ? (d < dmin ? d : dmin) : d;
                        dmax = cnt ? (d > dmax ? d : dmax) : d;
                        s1 += d;
                        s2 += d * d;
                        ++cnt;
                    }
                }
            }
        }
        sm.ps1[tid] = s1;
        sm.ps2[tid] = s2;
        sm.pmin[tid] = cnt ? dmin : __builtin_inf();
        sm.pmax[tid] = cnt ? dmax : -__builtin_inf();
        sm.pcnt[tid] = cnt;
    }
    __syncthreads();
    int complete = 1;
    if (tid < kXcCols) {
        const int cnt = sm.pcnt[2 * tid] + sm.pcnt[2 * tid + 1];
        const double s1 = sm.ps1[2 * tid] + sm.ps1[2 * tid + 1];
        const double s2 = sm.ps2[2 * tid] + sm.ps2[2 * tid + 1];
        const double lo = sm.pmin[2 * tid] < sm.pmin[2 * tid + 1] ? sm.pmin[2 * tid]
                                                                  : sm.pmin[2 * tid + 1];
        const double hi = sm.pmax[2 * tid] > sm.pmax[2 * tid + 1] ? sm.pmax[2 * tid]
                                                                  : sm.pmax[2 * tid + 1];
        double mean = 0.0, scale = 0.0;
        if (cnt > 0 && hi > lo) {                          // a constant column stays exactly 0
            mean = s1 / (double)cnt;
            const double var = (s2 - s1 * mean) / (double)cnt;
            scale = var > 0.0 && __builtin_isfinite(var) ? 1.0 / __builtin_sqrt(var) : 1.0;
        }
        sm.mean[tid] = mean;
        sm.scale[tid] = scale;
        if (tid < ncol && sm.colid[tid] >= 0) complete = cnt == n;
    }
    const bool fast = __syncthreads_and(complete);

    // ---- pass 3: the products ------------------------------------------------------------------
    const int fi = lane & 15, kk = lane >> 4;
    const int jt0 = diag ? wave : 0;                       // diagonal block: tiles J >= I only
    const int64_t K = g.K;
    double* out = g.xc + di * K * K;
    // element (16 wave + kk + 4 r, 16 jt + fi) of the block: the lane's accumulator entry r
    auto emit = [&](int jt, int r, double N, double P, double Sa, double Sb, double Qa,
                    double Qb) {
        const int ci = 16 * wave + kk + 4 * r, cj = jbase + 16 * jt + fi;
        const int64_t gi = (int64_t)bi * kXcBlock + ci, gj = (int64_t)bj * kXcBlock + 16 * jt + fi;
        if (gi >= K || gj >= K || (diag && gi > gj)) return;
        const bool same = sm.colid[ci] == sm.colid[cj] && (!Z || sm.zrow[ci] == sm.zrow[cj]);
        const double v = xcorr_entry(N, P, Sa, Sb, Qa, Qb, same);
        out[gi * K + gj] = v;
        out[gj * K + gi] = v;
    };
    const d4 zero4 = d4{0.0, 0.0, 0.0, 0.0};
    if (fast) {
        d4 P[kXcTiles], Sa = zero4, Qa = zero4, Sb = zero4, Qb = zero4;
#pragma unroll
        for (int jt = 0; jt < kXcTiles; ++jt) P[jt] = zero4;
        for (int r0 = 0; r0 < n; r0 += kXcRows) {
            __syncthreads();
            stage(r0, [&](int cc, int r, bool present, double d) {
                sm.tile[cc][r] = present ? (d - sm.mean[cc]) * sm.scale[cc] : 0.0;
            });
            __syncthreads();
            const int nks = n - r0 < kXcRows ? (n - r0 + 3) / 4 : kXcRows / 4;
            for (int it = 0; it < nks; ++it) {
                const int row = 4 * it + kk;
                const double ua = sm.tile[16 * wave + fi][row];
                const double ub = sm.tile[jbase + 16 * wave + fi][row];   // sums of tile column w
                double uj[kXcTiles];
#pragma unroll
                for (int jt = 0; jt < kXcTiles; ++jt) uj[jt] = sm.tile[jbase + 16 * jt + fi][row];
                Sa = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, 1.0, Sa, 0, 0, 0);
                Qa = __builtin_amdgcn_mfma_f64_16x16x4f64(ua * ua, 1.0, Qa, 0, 0, 0);
                Sb = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, ub, Sb, 0, 0, 0);
                Qb = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, ub * ub, Qb, 0, 0, 0);
#pragma unroll
                for (int jt = 0; jt < kXcTiles; ++jt)
                    if (jt >= jt0)
                        P[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, uj[jt], P[jt], 0, 0, 0);
            }
        }
        // the sums of block BJ's columns: tile column w from wave w (every accumulator row of a
        // lane holds the sum of column fi)
        __syncthreads();
        if (kk == 0) {
            sm.sb[16 * wave + fi] = Sb[0];
            sm.qb[16 * wave + fi] = Qb[0];
        }
        __syncthreads();
        const double N = (double)n;
#pragma unroll
        for (int jt = 0; jt < kXcTiles; ++jt) {
            if (jt < jt0) continue;
            const double sbj = sm.sb[16 * jt + fi], qbj = sm.qb[16 * jt + fi];
#pragma unroll
            for (int r = 0; r < 4; ++r) emit(jt, r, N, P[jt][r], Sa[r], sbj, Qa[r], qbj);
        }
    } else {
        // two tile columns at a time (12 accumulator tiles): the rows are staged once per half, and
        // the registers this saves let three workgroups share a CU.  A tile's sums do not depend
        // on which half it is in.  Every wave stages both halves (the barriers are the
        // workgroup's); a diagonal block's lower tiles only skip their MFMAs.
        constexpr int kHalf = kXcTiles / 2;
        for (int h = 0; h < 2; ++h) {
            d4 N[kHalf], P[kHalf], Sa[kHalf], Sb[kHalf], Qa[kHalf], Qb[kHalf];
#pragma unroll
            for (int j = 0; j < kHalf; ++j) {
                N[j] = zero4;
                P[j] = zero4;
                Sa[j] = zero4;
                Sb[j] = zero4;
                Qa[j] = zero4;
                Qb[j] = zero4;
            }
            for (int r0 = 0; r0 < n; r0 += kXcRows) {
                __syncthreads();
                stage(r0, [&](int cc, int r, bool present, double d) {
                    const double u = (d - sm.mean[cc]) * sm.scale[cc];
                    sm.tile[cc][r] = present && __builtin_isfinite(d) && __builtin_isfinite(u)
                                         ? u : qnan();     // NaN in the tile: missing
                });
                __syncthreads();
                const int nks = n - r0 < kXcRows ? (n - r0 + 3) / 4 : kXcRows / 4;
                for (int it = 0; it < nks; ++it) {
                    const int row = 4 * it + kk;
                    const double va = sm.tile[16 * wave + fi][row];
                    const bool fa = va == va;
                    const double ua = fa ? va : 0.0, ma = fa ? 1.0 : 0.0, qa = ua * ua;
#pragma unroll
                    for (int j = 0; j < kHalf; ++j) {
                        const int jt = kHalf * h + j;
                        if (jt < jt0) continue;
                        const double vb = sm.tile[jbase + 16 * jt + fi][row];
                        const bool fb = vb == vb;
                        const double ub = fb ? vb : 0.0, mb = fb ? 1.0 : 0.0, qb = ub * ub;
                        N[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma, mb, N[j], 0, 0, 0);
                        P[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, ub, P[j], 0, 0, 0);
                        Sa[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, mb, Sa[j], 0, 0, 0);
                        Sb[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma, ub, Sb[j], 0, 0, 0);
                        Qa[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa, mb, Qa[j], 0, 0, 0);
                        Qb[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma, qb, Qb[j], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kHalf; ++j) {
                const int jt = kHalf * h + j;
                if (jt < jt0) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    emit(jt, r, N[j][r], P[j][r], Sa[j][r], Sb[j][r], Qa[j][r], Qb[j][r]);
            }
        }
    }
}

// ---- summary: n, mean r, mean |r| of every pair over the dates --------------------------------
__global__ __launch_bounds__(64) void xcorr_summary_kernel(const double* xc, int64_t nd, int K,
                                                           double* stats) {
    const int64_t KK = (int64_t)K * K;
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= KK) return;
    int64_t n = 0;
    for (int64_t i = 0; i < nd; ++i) {
        const double v = xc[i * KK + p];
        n += v == v;
    }
    double mean = qnan(), mabs = qnan();
    if (n > 0) {
        auto val = [&](int64_t i) {
            const double v = xc[i * KK + p];
            return v == v ? v : 0.0;
        };
        auto aval = [&](int64_t i) {
            const double v = xc[i * KK + p];
            return v == v ? __builtin_fabs(v) : 0.0;
        };
        mean = seq_np_sum_of(val, nd) / (double)n;
        mabs = seq_np_sum_of(aval, nd) / (double)n;
    }
    stats[p * 3] = (double)n;
    stats[p * 3 + 1] = mean;
    stats[p * 3 + 2] = mabs;
}

}  // namespace
}  // namespace afm

using namespace afm;

extern "C" int afm_screen_xcorr_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                                    int64_t lda, const int32_t* cols, int K, const double* zs,
                                    const int32_t* zcols, const int32_t* dates, int64_t nd,
                                    const double* rows, const int32_t* rows_idx,
                                    const int32_t* nrows, double* xc) {
    AFM_CTX(ctx);
    (void)rows;                                            // afm_screen_ic_f64's shape; not read
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(T > 0 && lda > 0 && lda % 64 == 0 && col_stride >= 0,
                  "bad shape (lda a positive multiple of 64)");
    AFM_CHECK_ARG(base && cols && dates && rows_idx && nrows && xc, "null buffer");
    AFM_CHECK_ARG(zs || !zcols, "zcols without zs");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    const int64_t nblocks = ((int64_t)K + kXcBlock - 1) / kXcBlock;
    const int64_t npairs = nblocks * (nblocks + 1) / 2;
    AFM_CHECK_ARG(npairs < (1ll << 31) && nd * npairs < (1ll << 31),
                  "nd * B (B + 1) / 2 must be below 2^31 (B = ceil(K / 64))");
    if (nd == 0) return AFM_OK;
    XcorrArgs g{base, col_stride, T, lda, cols, K, zs, zcols, dates, (int)nblocks, (int)npairs,
                rows_idx, nrows, xc};
    const dim3 grid((unsigned)(nd * npairs)), block(kXcThreads);
    if (zs) hipLaunchKernelGGL(xcorr_kernel<true>, grid, block, 0, ctx->stream, g);
    else hipLaunchKernelGGL(xcorr_kernel<false>, grid, block, 0, ctx->stream, g);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_screen_xcorr_summary_f64(afm_ctx* ctx, const double* xc, int64_t nd, int K,
                                            double* stats) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(stats && (xc || nd == 0), "null buffer");
    const int64_t KK = (int64_t)K * K;
    AFM_CHECK_ARG(KK < (1ll << 31), "K * K must be below 2^31");
    hipLaunchKernelGGL(xcorr_summary_kernel, dim3((unsigned)((KK + 63) / 64)), dim3(64), 0,
                       ctx->stream, xc, nd, K, stats);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
