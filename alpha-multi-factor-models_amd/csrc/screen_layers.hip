// The backtest half of the factor screen (include/afm_screen_layers.h): decile layered returns,
// long-short spreads and the factor-weighted top-10 return of K factor columns on one shared row
// set -- the reference's _calc_layered_ret (KKT:324-340) and _backtest_top_stocks (KKT:356-375)
// of every column without the K-fold repetition of the forward returns, the merge / dropna
// cascade, the demeans and a full-grid sort.
//
//  screen_layers_kernel        one workgroup per (date, column), the columns of a date on
//                              consecutive workgroup ids (they share the date's three return
//                              planes and its rows_idx in L2).  Three phases:
//                                1. gather: the column's values at the date's rows (z-scored on
//                                   the way when zs is given, screen_ic_kernel's expression) into
//                                   register-resident order keys; a NaN value has no key.
//                                2. select: afm_order.h's decile select -- nine decile bounds and
//                                   the 10th largest of the n_k keyed rows in the same eight byte
//                                   passes, ties by position -- gives every row its layer (to
//                                   LDS, one byte per row) and the top-10 rows their rank.
//                                3. means: the three return planes go through LDS in chunks of
//                                   kSlChunk rows, each chunk sorted by layer (row order kept
//                                   inside a layer), and 30 lanes of wave 0 run xs_stats_kernel's
//                                   Kahan chains (return, layer), each over its contiguous run.
//                              Three instantiations by the date's row count: up to kSlFewRows
//                              rows kSlFewKeys keys per thread (128 VGPRs: two workgroups per
//                              CU, so one's serial means overlap the other's select), up to
//                              kSlSelectRows rows kSlSmallKeys, above that kSlLargeKeys; a
//                              workgroup of another instantiation leaves at once, and a grid
//                              launches only those its lda can need.
//  screen_port_kernel          one thread per (date, column, return): the top-10 cells of the
//                              item summed in the pivot's column order, which needs the
//                              column's pivot width min(10, max over dates of n_k) -- an atomic
//                              maximum the first kernel leaves.
//  screen_layer_series_kernel  one thread per (column, return, layer pair | top-k): the
//                              cumulative sums over the dates and the long-short differences
//                              (xs_series_kernel's rule: NaN stays NaN, the sum carries on).
#include "afm_internal.h"
#include "afm_screen_layers.h"

#pragma clang fp contract(off)

#include "afm_np_sum.h"
#include "afm_order.h"                 // okey, decile_select

namespace afm {
namespace {

constexpr int kSlThreads = 512;                    // threads per (date, column) workgroup
constexpr int kSlFewKeys = 8;                      // register keys per thread, dates of few rows
constexpr int kSlSmallKeys = 24;                   // ... of more
constexpr int kSlLargeKeys = 64;                   // ... and of many
constexpr int kSlFewRows = 4096;                   // row count up to which the few-key select runs
constexpr int kSlSelectRows = 12288;               // ... and the small one
constexpr int kSlMaxRows = 32768;                  // lda limit (afm_xs_prepare_f64's)
constexpr int kSlChunk = 512;                      // rows per staging chunk of the return planes
constexpr int kSlBatch = 8;                        // gathered rows of a thread in flight together
constexpr int kSlTopK = 10;
constexpr int kSlLayers = kOrdLayers;
constexpr int kSlWaves = kSlThreads / 64;
constexpr int kSlCells = 4 * kSlTopK;              // scratch doubles per item: f, r1, r2, r5
static_assert(kSlFewKeys * kSlThreads == kSlFewRows, "few-key select capacity");
static_assert(kSlSmallKeys * kSlThreads == kSlSelectRows, "small select capacity");
static_assert(kSlLargeKeys * kSlThreads == kSlMaxRows && kSlLargeKeys <= 64, "large capacity");
static_assert(kSlChunk == kSlThreads, "one staged row per thread");
static_assert(kSlFewKeys % kSlBatch == 0 && kSlSmallKeys % kSlBatch == 0 &&
                  kSlLargeKeys % kSlBatch == 0, "whole batches");
static_assert(kSlMaxRows <= 65536, "positions are selected in two byte passes");
static_assert(kSlTopK == kSelTop, "the select's last target is the book's last row");

struct SlArgs {
    const double* base;       // plane k: base + cols[k] * col_stride, [T][lda]
    int64_t col_stride, T, lda;
    const int32_t* cols;      // [K]
    int K;
    const double* zs;         // [..][lda][2] {mu, 1/sd}, or null: raw values
    const int32_t* zcols;     // [K] zs row of each column (null: row k)
    const int32_t* dates;     // [nd]
    const double* rows;       // [4][T][lda]: planes 1..3 the demeaned returns
    const int32_t* rows_idx;  // [T][lda]
    const int32_t* nrows;     // [T]
    double* layer_mean;       // [nd][K][3][10]
    int32_t* layer_cnt;       // [nd][K][10]
    double* cells;            // [nd][K][4][10]: factor and returns of the rows of rank 1..10
    int32_t* nmax;            // [K]: max over the dates of n_k
};

struct SlSelect {
    DecileSelect sel;
    int nk;
    int ntop;
    int wcnt[kSlWaves][kSlLayers];        // rows of each layer in each wave's 64 rows of a chunk
    int woff[kSlWaves][kSlLayers];        // where those go in the layer-sorted chunk
    int lend[kSlLayers];                  // the end of each layer's run
    u64 topk[kSlTopK];
    int topi[kSlTopK];
};

// NR: register keys per thread.  The workgroup takes the dates with lo < nrows <= NR * kSlThreads
// (and, for lo < 0, the dates without rows).  The few-key instantiation is held to the registers
// of four waves per SIMD (two workgroups per CU).
template <int NR, bool Z>
__global__ __launch_bounds__(kSlThreads, NR <= kSlFewKeys ? 4 : 2) void screen_layers_kernel(
    SlArgs g, int lo) {
    __shared__ SlSelect sh;
    __shared__ int8_t slay[NR * kSlThreads];               // layer - 1 of every row, -1: no key
    __shared__ double sret[3][kSlChunk];
    __shared__ double scell[4][kSlTopK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t item = blockIdx.x;
    const int64_t di = item / g.K;
    const int k = (int)(item % g.K);
    const int64_t t = g.dates[di];
    const int n = min(max(g.nrows[t], 0), (int)g.lda);
    if (n <= lo || n > NR * kSlThreads) return;            // the other instantiation's date
    const int64_t plane = g.T * g.lda, base = t * g.lda;
    const double* col = g.base + (int64_t)g.cols[k] * g.col_stride + base;
    const double2* zs2 = Z ? reinterpret_cast<const double2*>(g.zs) +
                                 (int64_t)(g.zcols ? g.zcols[k] : k) * g.lda
                           : nullptr;
    auto value = [&](int e) {                              // screen_ic_kernel's value of a row
        const int a = g.rows_idx[base + e];
        double v = col[a];
        if constexpr (Z) {
            const double2 m = zs2[a];
            v = (v - m.x) * m.y;
        }
        return v;
    };
    // ---- 1. gather: keys in registers; bit j of `keyed`: row j * kSlThreads + tid has one ----
    u64 ks[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) ks[j] = 0ull;
    u64 keyed = 0ull;
    if (tid == 0) { sh.nk = 0; sh.ntop = 0; }
    if (tid < kSlCells) scell[tid / kSlTopK][tid % kSlTopK] = qnan();
    __syncthreads();
    // (batches of kSlBatch rows per thread: the index loads, then the dependent value loads, all
    // of a batch in flight together; a thread without a row reads the date's first row instead)
#pragma unroll
    for (int j0 = 0; j0 < NR; j0 += kSlBatch) {
        if (j0 * kSlThreads >= n) break;                   // (uniform)
        int a[kSlBatch];
#pragma unroll
        for (int u = 0; u < kSlBatch; ++u) {
            const int e = (j0 + u) * kSlThreads + tid;
            a[u] = g.rows_idx[base + (e < n ? e : 0)];
        }
        double x[kSlBatch];
        double2 m[Z ? kSlBatch : 1];
#pragma unroll
        for (int u = 0; u < kSlBatch; ++u) {
            x[u] = col[a[u]];
            if constexpr (Z) m[u] = zs2[a[u]];
        }
#pragma unroll
        for (int u = 0; u < kSlBatch; ++u) {
            const int j = j0 + u, e = j * kSlThreads + tid;
            double v = x[u];
            if constexpr (Z) v = (v - m[u].x) * m[u].y;    // as the Gram and predict producers
            const bool ok = e < n && v == v;
            ks[j] = ok ? okey(v) : 0ull;
            keyed |= ok ? 1ull << j : 0ull;
            if (e < n) slay[e] = -1;
        }
    }
    {
        int c = __popcll(keyed);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
        if (lane == 0 && c) atomicAdd(&sh.nk, c);
    }
    __syncthreads();
    const int nk = sh.nk;
    double* lm = g.layer_mean + item * 3 * kSlLayers;
    int32_t* lc = g.layer_cnt + item * kSlLayers;
    double* cells = g.cells + item * kSlCells;
    if (nk == 0) {                                         // no ranked row: nothing but NaN
        if (tid < 3 * kSlLayers) lm[tid] = qnan();
        if (tid < kSlLayers) lc[tid] = 0;
        if (tid < kSlCells) cells[tid] = qnan();
        return;
    }
    // ---- 2. select (afm_order.h's decile select over the keyed rows) --------------------------
    if (tid == 0) atomicMax(g.nmax + k, nk);
    decile_select<NR, kSlThreads, 8>(sh.sel, ks, keyed, nk, tid);
    // every row's layer = 1 + the decile bounds below it; the top rows (key descending, position
    // ascending, up to the 10th)
    {
        u64 kq[kSelTargets];
        int iq[kSelTargets];
        bool has[kSelTargets];
#pragma unroll
        for (int q = 0; q < kSelTargets; ++q) {
            kq[q] = sh.sel.prefix[q];
            iq[q] = sh.sel.eqidx[q];
            has[q] = sh.sel.rneed[q] > 0;
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int e = j * kSlThreads + tid;
            if ((keyed >> j) & 1) {
                int l = 0;
#pragma unroll
                for (int q = 0; q < kSelTargets - 1; ++q)
                    l += !has[q] || ks[j] > kq[q] || (ks[j] == kq[q] && e > iq[q]) ? 1 : 0;
                slay[e] = (int8_t)l;
                const u64 kd = ~ks[j];                     // descending order key
                const int q = kSelTargets - 1;
                if (kd < kq[q] || (kd == kq[q] && e <= iq[q])) {
                    const int s = atomicAdd(&sh.ntop, 1);
                    if (s < kSlTopK) {
                        sh.topk[s] = kd;
                        sh.topi[s] = e;
                    }
                }
            }
        }
    }
    __syncthreads();
    const int ntop = min(sh.ntop, kSlTopK);
    if (tid < ntop) {                                      // rank among the top rows by counting
        const u64 mk = sh.topk[tid];
        const int mi = sh.topi[tid];
        int rk = 0;
        for (int f = 0; f < ntop; ++f)
            rk += sh.topk[f] < mk || (sh.topk[f] == mk && sh.topi[f] < mi);
        scell[0][rk] = value(mi);
#pragma unroll
        for (int q = 0; q < 3; ++q) scell[1 + q][rk] = g.rows[(1 + q) * plane + base + mi];
    }
    // ---- 3. the layer means: xs_stats_kernel's Kahan chains, lane = (return k1, layer l1) ------
    // A chunk's returns are written to LDS sorted by layer, rows of a layer in row order: a row's
    // place is its layer's start + the rows of the layer in earlier waves + those in earlier
    // lanes of its own wave (ballots).  A chain then reads one contiguous run, eight values per
    // wait, instead of one LDS round trip per row inside its dependency chain.
    const int k1 = lane / kSlLayers, l1 = lane % kSlLayers;
    double lsum = 0, lcomp = 0;
    int lcnt = 0;
    auto step = [&](double vx) {
        if (vx == vx) {
            lcnt += 1;
            const double y = vx - lcomp;
            const double tt = lsum + y;
            lcomp = tt - lsum - y;
            if (lcomp != lcomp) lcomp = 0;
            lsum = tt;
        }
    };
    double rv[3];
    auto load_chunk = [&](int c0) {
        const int64_t o = base + min(c0 + tid, n - 1);
#pragma unroll
        for (int q = 0; q < 3; ++q) rv[q] = g.rows[(1 + q) * plane + o];
    };
    load_chunk(0);
    for (int c0 = 0; c0 < n; c0 += kSlChunk) {
        const int len = min(kSlChunk, n - c0);
        const int myl = tid < len ? slay[c0 + tid] : -1;
        u64 mine = 0ull;
        int wcnt = 0;
#pragma unroll
        for (int l = 0; l < kSlLayers; ++l) {
            const u64 m = __ballot(myl == l);
            if (l == myl) mine = m;
            if (l == lane) wcnt = __popcll(m);
        }
        const int before = __popcll(mine & ((1ull << lane) - 1ull));
        if (lane < kSlLayers) sh.wcnt[wave][lane] = wcnt;
        __syncthreads();                                   // (the previous chunk is consumed)
        if (tid < kSlWaves * kSlLayers) {
            const int w = tid / kSlLayers, l = tid % kSlLayers;
            int off = 0;
            for (int u = 0; u < kSlWaves; ++u) {
                for (int v = 0; v < l; ++v) off += sh.wcnt[u][v];
                if (u < w) off += sh.wcnt[u][l];
            }
            sh.woff[w][l] = off;
            if (w == kSlWaves - 1) sh.lend[l] = off + sh.wcnt[w][l];
        }
        __syncthreads();
        if (myl >= 0) {
            const int p = sh.woff[wave][myl] + before;
#pragma unroll
            for (int q = 0; q < 3; ++q) sret[q][p] = rv[q];
        }
        __syncthreads();
        if (c0 + kSlChunk < n) load_chunk(c0 + kSlChunk);
        if (wave == 0 && lane < 3 * kSlLayers) {
            const double* R = sret[k1];
            int i = sh.woff[0][l1];
            const int end = sh.lend[l1];
            for (; i + 8 <= end; i += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = R[i + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) step(v[u]);
            }
            for (; i < end; ++i) step(R[i]);
        }
    }
    if (wave == 0 && lane < 3 * kSlLayers) {
        lm[k1 * kSlLayers + l1] = lcnt ? lsum / (double)lcnt : qnan();
        if (k1 == 0) lc[l1] = lcnt;
    }
    if (tid < kSlCells) cells[tid] = scell[tid / kSlTopK][tid % kSlTopK];
}

// port of (item, return q): xs_stats_kernel's factor-weighted sum over the pivot's columns
__global__ __launch_bounds__(256) void screen_port_kernel(int64_t items, int K,
                                                          const double* cells,
                                                          const int32_t* nmax, double* port) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= items * 3) return;
    const int64_t item = id / 3;
    const int q = (int)(id % 3);
    const double* pf = cells + item * kSlCells;
    const double* pr = pf + (1 + q) * kSlTopK;
    if (pf[0] != pf[0]) {                                  // no row of rank 1: n_k == 0
        port[id] = qnan();
        return;
    }
    // pivot columns in string order '1.0','10.0','2.0',...,'9.0' (or 1..m for m < 10)
    const int m = min(nmax[item % K], kSlTopK);
    int order[kSlTopK];
    if (m >= 10) {
        order[0] = 1; order[1] = 10;
        for (int j = 2; j < 10; ++j) order[j] = j;
    } else {
        for (int j = 0; j < m; ++j) order[j] = j + 1;
    }
    double row[kSlTopK];
    for (int j = 0; j < m; ++j) {
        const double f = pf[order[j] - 1];                 // NaN: the date has no row of the rank
        row[j] = f == f ? f : 0.0;
    }
    const double wsum = leaf_sum(row, m);
    for (int j = 0; j < m; ++j) {
        const int c = order[j] - 1;
        double v = qnan();
        if (pf[c] == pf[c]) v = pr[c] * (pf[c] / wsum);
        row[j] = v == v ? v : 0.0;
    }
    port[id] = leaf_sum(row, m);
}

// ---- series ------------------------------------------------------------------------------------
// Task (k, q, j): j < 5 the layers j + 1 and 10 - j with their long-short difference, j == 5 the
// top-k return.  A thread's inputs are read in batches of kSlSerB dates, all issued before the
// batch's dependent sums (xs_series_kernel's scheme).
constexpr int kSlSerB = 16;

__global__ __launch_bounds__(64) void screen_layer_series_kernel(int64_t nd, int K,
                                                                 const double* layer_mean,
                                                                 const double* port,
                                                                 double* cum_layer, double* ls,
                                                                 double* cum_port) {
    const int64_t task = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (task >= (int64_t)K * 18) return;
    const int64_t kq = task / 6;                           // k * 3 + q
    const int j = (int)(task % 6);
    const int64_t K3 = (int64_t)K * 3;
    if (j == 5) {
        double s = 0.0;
        for (int64_t i0 = 0; i0 < nd; i0 += kSlSerB) {
            double xb[kSlSerB];
#pragma unroll
            for (int u = 0; u < kSlSerB; ++u)
                xb[u] = i0 + u < nd ? port[(i0 + u) * K3 + kq] : 0.0;
#pragma unroll
            for (int u = 0; u < kSlSerB; ++u) {
                if (i0 + u >= nd) break;
                double* o = &cum_port[(i0 + u) * K3 + kq];
                if (xb[u] == xb[u]) {
                    s = s + xb[u];
                    *o = s;
                } else {
                    *o = qnan();
                }
            }
        }
        return;
    }
    const int lo = j, hi = kSlLayers - 1 - j;
    double slo = 0.0, shi = 0.0;
    for (int64_t i0 = 0; i0 < nd; i0 += kSlSerB) {
        double xl[kSlSerB], xh[kSlSerB];
#pragma unroll
        for (int u = 0; u < kSlSerB; ++u) {
            const int64_t o = ((i0 + u < nd ? i0 + u : nd - 1) * K3 + kq) * kSlLayers;
            xl[u] = layer_mean[o + lo];
            xh[u] = layer_mean[o + hi];
        }
#pragma unroll
        for (int u = 0; u < kSlSerB; ++u) {
            if (i0 + u >= nd) break;
            const int64_t o = (i0 + u) * K3 + kq;
            double cl = qnan(), ch = qnan();
            if (xl[u] == xl[u]) {
                slo = slo + xl[u];
                cl = slo;
            }
            if (xh[u] == xh[u]) {
                shi = shi + xh[u];
                ch = shi;
            }
            cum_layer[o * kSlLayers + lo] = cl;
            cum_layer[o * kSlLayers + hi] = ch;
            ls[o * 5 + j] = ch - cl;
        }
    }
}

template <int NR>
void launch_layers(const SlArgs& g, int lo, unsigned grid, hipStream_t stream) {
    if (g.zs)
        hipLaunchKernelGGL((screen_layers_kernel<NR, true>), dim3(grid), dim3(kSlThreads), 0,
                           stream, g, lo);
    else
        hipLaunchKernelGGL((screen_layers_kernel<NR, false>), dim3(grid), dim3(kSlThreads), 0,
                           stream, g, lo);
}

}  // namespace
}  // namespace afm

using namespace afm;

extern "C" int afm_screen_layers_f64(afm_ctx* ctx, const double* base, int64_t col_stride,
                                     int64_t T, int64_t lda, const int32_t* cols, int K,
                                     const double* zs, const int32_t* zcols, const int32_t* dates,
                                     int64_t nd, const double* rows, const int32_t* rows_idx,
                                     const int32_t* nrows, double* layer_mean, int32_t* layer_cnt,
                                     double* port, double* scratch) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(T > 0 && lda > 0 && lda % 64 == 0 && col_stride >= 0,
                  "bad shape (lda a positive multiple of 64)");
    AFM_CHECK_ARG(lda <= kSlMaxRows, "lda must be at most 32768");
    AFM_CHECK_ARG(base && cols && dates && rows && rows_idx && nrows && layer_mean && layer_cnt &&
                      port && scratch, "null buffer");
    AFM_CHECK_ARG(zs || !zcols, "zcols without zs");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(nd < (1ll << 31) && nd * K < (1ll << 31), "nd * K must be below 2^31");
    if (nd == 0) return AFM_OK;
    const int64_t items = nd * K;
    double* cells = scratch;
    int32_t* nmax = reinterpret_cast<int32_t*>(scratch + items * kSlCells);
    AFM_HIP(hipMemsetAsync(nmax, 0, sizeof(int32_t) * (size_t)K, ctx->stream));
    SlArgs g{base, col_stride, T, lda, cols, K, zs, zcols, dates, rows, rows_idx, nrows,
             layer_mean, layer_cnt, cells, nmax};
    launch_layers<kSlFewKeys>(g, -1, (unsigned)items, ctx->stream);
    AFM_HIP(hipGetLastError());
    if (lda > kSlFewRows) {
        launch_layers<kSlSmallKeys>(g, kSlFewRows, (unsigned)items, ctx->stream);
        AFM_HIP(hipGetLastError());
    }
    if (lda > kSlSelectRows) {
        launch_layers<kSlLargeKeys>(g, kSlSelectRows, (unsigned)items, ctx->stream);
        AFM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(screen_port_kernel, dim3((unsigned)((items * 3 + 255) / 256)), dim3(256),
                       0, ctx->stream, items, K, cells, nmax, port);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_screen_layer_series_f64(afm_ctx* ctx, int64_t nd, int K,
                                           const double* layer_mean, const double* port,
                                           double* cum_layer, double* ls, double* cum_port) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(layer_mean && port && cum_layer && ls && cum_port, "null buffer");
    if (nd == 0) return AFM_OK;
    const int64_t tasks = (int64_t)K * 18;
    hipLaunchKernelGGL(screen_layer_series_kernel, dim3((unsigned)((tasks + 63) / 64)), dim3(64),
                       0, ctx->stream, nd, K, layer_mean, port, cum_layer, ls, cum_port);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
