// The stability half of the factor screen (include/afm_turnover.h): rank autocorrelation, the
// turnover of the extreme decile layers and the turnover of the factor-weighted top-10 book of K
// columns between evaluated date i and date i - lag, for up to eight lags -- a pair pass over two
// dates in two stages, all of it integer or fixed-order arithmetic.
//
//  turnover_marks_kernel    one workgroup per (evaluated date, column), once whatever the lags
//                           are.  The column's values gathered through rows_idx (z-scored on the
//                           way when zs is given), their order keys sorted run by run -- keys
//                           only, afm_order.h's run sort as in rank_ic_kernel, including the
//                           scratch path above kSortLdsRows rows; a NaN sorts as the pad key and
//                           has no rank --
//                           and every row finds the bounds [lb, ub) of its own key.  It leaves the
//                           date's marks in the caller's scratch:
//                             ranks   int32 [lda] by asset: 2 * rank = lb + ub + 1, 0 = no rank;
//                             top/bot bitmaps by asset of layer 10 and layer 1;
//                             book    the <= 10 (asset, weight) pairs of the top book, by asset.
//                           method='first' decides only at three bounds (the end of layer 1, the
//                           start of layer 10, the 10th largest): a row whose [lb, ub) lies on one
//                           side is decided by its bounds, the rows of the one key that straddles
//                           a bound by counting the straddling rows at earlier positions -- a
//                           ballot and a scan over the waves, chunk by chunk in row order.
//                           Instantiated by the rows a thread holds (kTvFewKeys / kTvMidKeys /
//                           kTvManyKeys, chosen from lda): the rows' packed bounds stay in
//                           registers between the two phases.
//  turnover_pairs_kernel    one wave per (date, column, lag): the two int32 rank rows read in
//                           coalesced 16-byte pieces into six int64 sums over the assets ranked on
//                           both dates, popcounts of top1 & ~top0 and bot1 & ~bot0, and lane 0
//                           merges the two books in ascending asset order.  No floating-point
//                           reduction: the correlation is formed from exact integers, the book
//                           sum is serial.
//  turnover_summary_kernel  one thread per (column, lag, series): n and the mean over the dates in
//                           order (xcorr_summary_kernel's shape).
//
// The marks of all dates would be nd * K * (lda / 2 + ...) words (5.2 GB at 97 columns, 4,112
// dates, lda 3,008), so the scratch holds kTvBudget bytes of date slots used as a ring: the dates
// are taken in blocks, marks then pairs, a block and the largest near lag before it resident.  A
// lag longer than half the ring is paired afterwards block by block with both sides' marks
// computed again.  Both routes run the same two kernels on the same inputs, so an item's bits do
// not depend on the route.
#include "afm_internal.h"
#include "afm_turnover.h"

#pragma clang fp contract(off)

#include "afm_np_sum.h"                // qnan
#include "afm_order.h"                 // okey, layer_of, sort_rows, bounds

namespace afm {
namespace {

constexpr int kTvThreads = 1024;       // 16 waves
constexpr int kTvWaves = kTvThreads / 64;
constexpr int kTvMaxRows = 32768;      // afm_xs_prepare_f64's limit
constexpr int kTvFewKeys = 4;          // rows per thread: lda up to 4096
constexpr int kTvMidKeys = 16;         // ... up to 16384
constexpr int kTvManyKeys = 32;        // ... up to 32768
constexpr int kTvSlots = 256;          // workgroups of a marks launch that sorts through scratch
constexpr int kTvBook = 10;            // rows of the top book
constexpr int kTvHeader = 16;          // words: {nbook | n_k << 32}, 10 weights, 5 of assets
constexpr i64 kTvBudget = 128ll << 20; // bytes of date slots in the scratch (at least two slots)
constexpr int kTvPairThreads = 256;    // four items a workgroup
constexpr unsigned kTvNoKey = ~0u;
static_assert(kTvThreads == kSortThreads, "afm_order.h's sort is written for this workgroup");
static_assert(kTvManyKeys * kTvThreads == kTvMaxRows && kTvMidKeys * kTvThreads == kSortLdsRows,
              "key capacities");
static_assert(kTvMaxRows <= 65535 + 1, "bounds are packed in 16 bits each");

// ---- marks -----------------------------------------------------------------------------------------
// words of one (date, column) record: ranks, two bitmaps, the header
__host__ __device__ __forceinline__ int64_t rec_words(int64_t lda) {
    return lda / 2 + ((lda / 32 + kTvHeader + 7) & ~(int64_t)7);
}

struct TvMarksArgs {
    const double* base;       // plane k: base + cols[k] * col_stride, [T][lda]
    int64_t col_stride, T, lda;
    const int32_t* cols;      // [K]
    int K;
    const double* zs;         // [..][lda][2] {mu, 1/sd}, or null: raw values
    const int32_t* zcols;     // [K] zs row of each column (null: row k)
    const int32_t* dates;     // [nd]
    int64_t i0, items;        // positions [i0, i0 + items / K)
    int64_t add, mod;         // the slot of position i: (i - i0 + add) % mod
    const int32_t* rows_idx;  // [T][lda]
    const int32_t* nrows;     // [T]
    u64* sortscr;             // [gridDim.x][lda] when lda > kSortLdsRows
    u64* marks;               // [mod][K][rec_words(lda)]
};

struct TvShared {
    int wc[2][kTvWaves][3];   // straddling rows of each wave in a chunk (bot, top, book)
    int R1, R9;               // the last first-rank of layer 1 and of layer 9
    int nbook;
    int bke[kTvBook], bkl[kTvBook], bka[kTvBook];   // row, lb and asset of the book's rows
    double bkf[kTvBook];
};

template <int NR, bool Z>
__global__ __launch_bounds__(kTvThreads) void turnover_marks_kernel(TvMarksArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ TvShared sh;
    __shared__ unsigned sbm[2][kTvMaxRows / 32];           // top, bot by asset
    u64* lds = reinterpret_cast<u64*>(dyn);
    u64* scr = g.sortscr ? g.sortscr + (int64_t)blockIdx.x * g.lda : nullptr;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lda = (int)g.lda;
    const double2* zs2 = reinterpret_cast<const double2*>(g.zs);
    const int64_t rec = rec_words(g.lda);
    for (int64_t item = blockIdx.x; item < g.items; item += gridDim.x) {
        const int k = (int)(item % g.K);
        const int64_t ii = item / g.K;
        const int64_t t = g.dates[g.i0 + ii];
        const int n = min(max(g.nrows[t], 0), min(lda, NR * kTvThreads));
        const int64_t base = t * g.lda;
        const double* col = g.base + (int64_t)g.cols[k] * g.col_stride + base;
        const double2* zrow = Z ? zs2 + (int64_t)(g.zcols ? g.zcols[k] : k) * g.lda : nullptr;
        const int32_t* idx = g.rows_idx + base;
        u64* out = g.marks + (((ii + g.add) % g.mod) * g.K + k) * rec;
        int32_t* rk = reinterpret_cast<int32_t*>(out);
        u64* bits = out + lda / 2;                         // top [lda / 64], then bot
        u64* hdr = bits + lda / 32;
        auto asset = [&](int e) { return min(max(idx[e], 0), lda - 1); };
        auto fval = [&](int e) {                           // rank_ic_kernel's value of a row
            const int a = asset(e);
            double x = col[a];
            if constexpr (Z) {
                const double2 m = zrow[a];
                x = (x - m.x) * m.y;
            }
            return x;
        };
        __syncthreads();                                   // the previous item is written out
        for (int a = tid; a < lda; a += kTvThreads) rk[a] = 0;
        for (int w = tid; w < lda / 32; w += kTvThreads) {
            sbm[0][w] = 0u;
            sbm[1][w] = 0u;
        }
        if (tid == 0) sh.nbook = 0;
        sort_rows(lds, scr, n, [&](int e) {
            const double v = fval(e);
            return v == v ? okey(v) : kSortPad;
        });
        int nk = 0;                                        // the ranked rows: the keys below the pad
        {
            int lb;                                        // (kSortPad - 1 is a NaN's key: no row's)
            bounds(lds, scr, n, kSortPad - 1, lb, nk);
        }
        if (nk == 0) {                                     // (uniform) nothing ranked
            for (int w = tid; w < lda / 32; w += kTvThreads) bits[w] = 0ull;
            if (tid < kTvHeader) hdr[tid] = 0ull;
            continue;
        }
        if (tid < 2) {                // the largest first-rank whose layer is <= 1 (tid 0), <= 9
            const int l = tid == 0 ? 1 : kOrdLayers - 1;
            int lo_ = 0, hi = nk;
            while (lo_ < hi) {
                const int m = (lo_ + hi + 1) >> 1;
                if (layer_of(m, nk) <= l) lo_ = m; else hi = m - 1;
            }
            if (tid == 0) sh.R1 = lo_; else sh.R9 = lo_;
        }
        // ---- every row's bounds; the doubled ranks by asset -----------------------------------
        unsigned pk[NR];                                   // lb | ub << 16
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int e = j * kTvThreads + tid;
            pk[j] = kTvNoKey;
            if (e < n) {
                const double v = fval(e);
                if (v == v) {
                    int lb, ub;
                    bounds(lds, scr, n, okey(v), lb, ub);
                    pk[j] = (unsigned)lb | (unsigned)ub << 16;
                    rk[asset(e)] = lb + ub + 1;
                }
            }
        }
        __syncthreads();
        // ---- layer 1, layer 10 and the book: method='first' at the three bounds ---------------
        const int R1 = sh.R1, R9 = sh.R9;
        int seen[3] = {0, 0, 0};                           // straddling rows of the earlier chunks
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (j * kTvThreads >= n) break;                // (uniform)
            const int e = j * kTvThreads + tid;
            const bool has = pk[j] != kTvNoKey;
            const int lb = (int)(pk[j] & 0xffffu), ub = (int)(pk[j] >> 16);
            const int dlo = nk - ub, dhi = nk - lb;        // descending first-rank in (dlo, dhi]
            const bool s0 = has && lb < R1 && R1 < ub;
            const bool s1 = has && lb < R9 && R9 < ub;
            const bool s2 = has && dlo < kTvBook && kTvBook < dhi;
            const u64 m0 = __ballot(s0), m1 = __ballot(s1), m2 = __ballot(s2);
            if (lane == 0) {
                sh.wc[j & 1][wave][0] = __popcll(m0);
                sh.wc[j & 1][wave][1] = __popcll(m1);
                sh.wc[j & 1][wave][2] = __popcll(m2);
            }
            __syncthreads();
            const u64 below = (1ull << lane) - 1ull;
            int eq[3] = {seen[0] + (int)__popcll(m0 & below), seen[1] + (int)__popcll(m1 & below),
                         seen[2] + (int)__popcll(m2 & below)};   // equal keys at earlier positions
            // (four waves' counts per wait: unrolled over all sixteen, each chunk's 48 counts stay
            // live beside the packed bounds and every instantiation spills)
#pragma unroll 4
            for (int w = 0; w < kTvWaves; ++w) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int c = sh.wc[j & 1][w][q];
                    seen[q] += c;
                    if (w < wave) eq[q] += c;
                }
            }
            if (has) {
                const int a = asset(e);
                if (ub <= R1 || (s0 && eq[0] < R1 - lb)) atomicOr(&sbm[1][a >> 5], 1u << (a & 31));
                if (lb >= R9 || (s1 && eq[1] >= R9 - lb)) atomicOr(&sbm[0][a >> 5], 1u << (a & 31));
                if (dhi <= kTvBook || (s2 && eq[2] < kTvBook - dlo)) {
                    const int s = atomicAdd(&sh.nbook, 1);
                    if (s < kTvBook) {
                        sh.bke[s] = e;
                        sh.bkl[s] = lb;
                        sh.bka[s] = a;
                    }
                }
            }
        }
        __syncthreads();
        for (int w = tid; w < lda / 32; w += kTvThreads) {
            const int b = w < lda / 64 ? 0 : 1, o = 2 * (w - b * (lda / 64));
            bits[w] = (u64)sbm[b][o] | (u64)sbm[b][o + 1] << 32;
        }
        const int nb = min(sh.nbook, kTvBook);
        if (tid < nb) sh.bkf[tid] = fval(sh.bke[tid]);
        __syncthreads();
        if (tid == 0) {
            // rank order: key descending (lb descending), ties by row position
            int ord[kTvBook];
            for (int s = 0; s < nb; ++s) {
                int r = 0;
                for (int f = 0; f < nb; ++f)
                    r += sh.bkl[f] > sh.bkl[s] || (sh.bkl[f] == sh.bkl[s] && sh.bke[f] < sh.bke[s]);
                ord[r] = s;
            }
            double S = 0.0;
            for (int r = 0; r < nb; ++r) S = S + sh.bkf[ord[r]];
            // by asset ascending for the pair kernel's merge
            u64 aw[(kTvBook + 1) / 2];
            for (int s = 0; s < (kTvBook + 1) / 2; ++s) aw[s] = 0ull;
            for (int s = 0; s < nb; ++s) {
                int r = 0;
                for (int f = 0; f < nb; ++f)
                    r += sh.bka[f] < sh.bka[s] || (sh.bka[f] == sh.bka[s] && f < s);
                hdr[1 + r] = (u64)__double_as_longlong(sh.bkf[s] / S);
                aw[r >> 1] |= (u64)(unsigned)sh.bka[s] << (32 * (r & 1));
            }
            for (int r = nb; r < kTvBook; ++r) hdr[1 + r] = 0ull;
            for (int s = 0; s < (kTvBook + 1) / 2; ++s) hdr[1 + kTvBook + s] = aw[s];
            hdr[0] = (u64)(unsigned)nb | (u64)(unsigned)nk << 32;
        }
    }
}

// ---- pairs -----------------------------------------------------------------------------------------
struct TvPairArgs {
    const u64* marks;         // [mod][K][rec_words(lda)]
    int64_t lda;
    int K, L;
    int64_t i0, items;        // positions [i0, i0 + items / (K * L)), item = ((i - i0) * K + k) * L + l
    int64_t mod;
    int64_t add1;             // the slot of t1 = position i: (i - i0 + add1) % mod
    int64_t add0[AFM_TURNOVER_MAX_LAGS];   // ... of t0 = position i - lag[l]: (i - i0 + add0[l]) % mod
    int lag[AFM_TURNOVER_MAX_LAGS];
    unsigned active;          // bit l: lag l is paired by this launch
    double* rank_ac;          // [nd][K][L]
    int32_t* counts;          // [nd][K][L][5]
    double* port_turn;        // [nd][K][L]
};

__device__ __forceinline__ i64 wave_sum(i64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                              // on lane 0
}

__global__ __launch_bounds__(kTvPairThreads) void turnover_pairs_kernel(TvPairArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * (kTvPairThreads / 64) + (threadIdx.x >> 6);
    if (item >= g.items) return;
    const int l = (int)(item % g.L);
    const int k = (int)((item / g.L) % g.K);
    const int64_t ii = item / ((int64_t)g.L * g.K);
    const int64_t i = g.i0 + ii;
    if (!((g.active >> l) & 1u) || i < g.lag[l]) return;   // (per wave)
    const int lda = (int)g.lda;
    const int64_t rec = rec_words(g.lda);
    const u64* m1 = g.marks + (((ii + g.add1) % g.mod) * g.K + k) * rec;
    const u64* m0 = g.marks + (((ii + g.add0[l]) % g.mod) * g.K + k) * rec;
    const int4* x4 = reinterpret_cast<const int4*>(m0);
    const int4* y4 = reinterpret_cast<const int4*>(m1);
    i64 n = 0, sx = 0, sy = 0, sxy = 0, sxx = 0, syy = 0;
    auto acc = [&](int x, int y) {
        if (x > 0 && y > 0) {
            n += 1;
            sx += x;
            sy += y;
            sxy += (i64)x * y;
            sxx += (i64)x * x;
            syy += (i64)y * y;
        }
    };
    for (int c = lane; c < lda / 4; c += 64) {
        const int4 x = x4[c], y = y4[c];
        acc(x.x, y.x);
        acc(x.y, y.y);
        acc(x.z, y.z);
        acc(x.w, y.w);
    }
    const u64* b1 = m1 + lda / 2;
    const u64* b0 = m0 + lda / 2;
    i64 ntop = 0, newtop = 0, nbot = 0, newbot = 0;
    const int bw = lda / 64;
    for (int w = lane; w < bw; w += 64) {
        const u64 t1 = b1[w], t0 = b0[w], o1 = b1[bw + w], o0 = b0[bw + w];
        ntop += __popcll(t1);
        newtop += __popcll(t1 & ~t0);
        nbot += __popcll(o1);
        newbot += __popcll(o1 & ~o0);
    }
    n = wave_sum(n);
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    sxy = wave_sum(sxy);
    sxx = wave_sum(sxx);
    syy = wave_sum(syy);
    ntop = wave_sum(ntop);
    newtop = wave_sum(newtop);
    nbot = wave_sum(nbot);
    newbot = wave_sum(newbot);
    // the two books, each ascending by asset: 20 lanes bring them to the wave's LDS, lane 0 merges
    __shared__ double swt[kTvPairThreads / 64][2][kTvBook];
    __shared__ int sas[kTvPairThreads / 64][2][kTvBook];
    const int wv = threadIdx.x >> 6;
    const u64* h1 = b1 + 2 * bw;
    const u64* h0 = b0 + 2 * bw;
    if (lane < 2 * kTvBook) {
        const int side = lane / kTvBook, s = lane % kTvBook;
        const u64* h = side ? h1 : h0;
        swt[wv][side][s] = __longlong_as_double((i64)h[1 + s]);
        sas[wv][side][s] = (int)(unsigned)(h[1 + kTvBook + (s >> 1)] >> (32 * (s & 1)));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (lane != 0) return;
    const int64_t o = (i * g.K + k) * g.L + l;
    double ac = qnan();
    if (n >= 2) {
        const i64 cxy = n * sxy - sx * sy, cxx = n * sxx - sx * sx, cyy = n * syy - sy * sy;
        const double root = __builtin_sqrt((double)cxx * (double)cyy);
        if (root != 0) ac = (double)cxy / root;
    }
    g.rank_ac[o] = ac;
    int32_t* cnt = g.counts + o * 5;
    cnt[0] = (int32_t)n;
    cnt[1] = (int32_t)ntop;
    cnt[2] = (int32_t)newtop;
    cnt[3] = (int32_t)nbot;
    cnt[4] = (int32_t)newbot;
    const int n1 = (int)(unsigned)h1[0], n0 = (int)(unsigned)h0[0];
    double turn = qnan();
    if (n0 > 0 && n1 > 0 && n0 <= kTvBook && n1 <= kTvBook) {
        const int* a1 = sas[wv][1];
        const int* a0 = sas[wv][0];
        const double* w1 = swt[wv][1];
        const double* w0 = swt[wv][0];
        bool fin = true;
        for (int s = 0; s < n1; ++s) fin = fin && __builtin_isfinite(w1[s]);
        for (int s = 0; s < n0; ++s) fin = fin && __builtin_isfinite(w0[s]);
        if (fin) {
            double s = 0.0;
            int p1 = 0, p0 = 0;
            while (p1 < n1 || p0 < n0) {
                double d;
                if (p0 >= n0 || (p1 < n1 && a1[p1] < a0[p0])) d = w1[p1++] - 0.0;
                else if (p1 >= n1 || a0[p0] < a1[p1]) d = 0.0 - w0[p0++];
                else d = w1[p1++] - w0[p0++];
                s = s + __builtin_fabs(d);
            }
            turn = 0.5 * s;
        }
    }
    g.port_turn[o] = turn;
}

// the items without an earlier date: i < lag
__global__ __launch_bounds__(256) void turnover_fill_kernel(TvPairArgs g, int64_t total) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int l = (int)(id % g.L);
    const int64_t i = id / ((int64_t)g.L * g.K);
    if (i >= g.lag[l]) return;
    g.rank_ac[id] = qnan();
    g.port_turn[id] = qnan();
    for (int c = 0; c < 5; ++c) g.counts[id * 5 + c] = 0;
}

// ---- summary ---------------------------------------------------------------------------------------
constexpr int kTvSumBatch = 16;

__global__ __launch_bounds__(64) void turnover_summary_kernel(int64_t nd, int K, int L,
                                                              const double* rank_ac,
                                                              const int32_t* counts,
                                                              const double* port_turn,
                                                              double* stats) {
    const int64_t task = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (task >= (int64_t)K * L * 4) return;
    const int s = (int)(task % 4);
    const int64_t kl = task / 4;                           // k * L + l
    const int64_t KL = (int64_t)K * L;
    double sum = 0.0;
    int64_t n = 0;
    // (a batch of dates is read before its dependent adds: screen_layer_series_kernel's scheme)
    for (int64_t i0 = 0; i0 < nd; i0 += kTvSumBatch) {
        double v[kTvSumBatch];
#pragma unroll
        for (int u = 0; u < kTvSumBatch; ++u) {
            const int64_t o = (i0 + u < nd ? i0 + u : nd - 1) * KL + kl;
            if (s == 0) v[u] = rank_ac[o];
            else if (s == 3) v[u] = port_turn[o];
            else {
                const int32_t den = counts[o * 5 + (s == 1 ? 1 : 3)];
                const int32_t num = counts[o * 5 + (s == 1 ? 2 : 4)];
                v[u] = den > 0 ? (double)num / (double)den : qnan();
            }
        }
#pragma unroll
        for (int u = 0; u < kTvSumBatch; ++u) {
            if (i0 + u < nd && v[u] == v[u]) {
                sum = sum + v[u];
                n += 1;
            }
        }
    }
    stats[task * 2] = (double)n;
    stats[task * 2 + 1] = n ? sum / (double)n : qnan();
}

// ---- host ------------------------------------------------------------------------------------------
bool tv_shape_ok(int64_t lda) { return lda > 0 && lda % 64 == 0 && lda <= kTvMaxRows; }

struct TvLayout {
    int64_t rec, slots, sort_words;
};

TvLayout tv_layout(int64_t nd, int K, int64_t lda) {
    TvLayout y;
    y.rec = rec_words(lda);
    const int64_t per_date = (int64_t)K * y.rec * (int64_t)sizeof(u64);
    y.slots = kTvBudget / per_date;
    if (y.slots < 2) y.slots = 2;
    if (y.slots > nd) y.slots = nd > 0 ? nd : 1;
    y.sort_words = lda > kSortLdsRows ? (int64_t)kTvSlots * lda : 0;
    return y;
}

template <int NR>
int launch_marks(afm_ctx* ctx, const TvMarksArgs& g) {
    const bool chunked = g.lda > kSortLdsRows;
    const dim3 grid((unsigned)(chunked && g.items > kTvSlots ? kTvSlots : g.items));
    const size_t lds = sizeof(u64) * (size_t)pow2_at_least((int)(g.lda < kSortLdsRows ? g.lda : kSortLdsRows));
    if (g.zs) {
        AFM_HIP(afm_lds_opt_in(ctx, (const void*)turnover_marks_kernel<NR, true>,
                               sizeof(u64) * kSortLdsRows));
        hipLaunchKernelGGL((turnover_marks_kernel<NR, true>), grid, dim3(kTvThreads), lds,
                           ctx->stream, g);
    } else {
        AFM_HIP(afm_lds_opt_in(ctx, (const void*)turnover_marks_kernel<NR, false>,
                               sizeof(u64) * kSortLdsRows));
        hipLaunchKernelGGL((turnover_marks_kernel<NR, false>), grid, dim3(kTvThreads), lds,
                           ctx->stream, g);
    }
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

// the marks of positions [i0, i1) into the slots (i - i0 + add) % mod
int marks(afm_ctx* ctx, TvMarksArgs g, int64_t i0, int64_t i1, int64_t add) {
    g.i0 = i0;
    g.items = (i1 - i0) * g.K;
    g.add = add;
    if (g.lda <= kTvFewKeys * kTvThreads) return launch_marks<kTvFewKeys>(ctx, g);
    if (g.lda <= kTvMidKeys * kTvThreads) return launch_marks<kTvMidKeys>(ctx, g);
    return launch_marks<kTvManyKeys>(ctx, g);
}

int pairs(afm_ctx* ctx, TvPairArgs g, int64_t i0, int64_t i1) {
    g.i0 = i0;
    g.items = (i1 - i0) * g.K * g.L;
    const int per = kTvPairThreads / 64;
    hipLaunchKernelGGL(turnover_pairs_kernel, dim3((unsigned)((g.items + per - 1) / per)),
                       dim3(kTvPairThreads), 0, ctx->stream, g);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

}  // namespace
}  // namespace afm

using namespace afm;

extern "C" int64_t afm_screen_turnover_scratch_bytes(int64_t nd, int K, int64_t lda) {
    if (!tv_shape_ok(lda) || nd < 0 || K < 1) {
        afm_set_error("afm_screen_turnover_scratch_bytes: lda must be a positive multiple of 64 up "
                      "to 32768, nd >= 0 and K >= 1");
        return -1;
    }
    const TvLayout y = tv_layout(nd, K, lda);
    return (y.slots * K * y.rec + y.sort_words) * (int64_t)sizeof(u64);
}

extern "C" int afm_screen_turnover_f64(afm_ctx* ctx, const double* base, int64_t col_stride,
                                       int64_t T, int64_t lda, const int32_t* cols, int K,
                                       const double* zs, const int32_t* zcols,
                                       const int32_t* dates, int64_t nd, const int32_t* rows_idx,
                                       const int32_t* nrows, const int32_t* lags, int L,
                                       double* rank_ac, int32_t* counts, double* port_turn,
                                       uint64_t* scratch) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(T > 0 && tv_shape_ok(lda) && col_stride >= 0,
                  "bad shape (lda a positive multiple of 64 up to 32768)");
    AFM_CHECK_ARG(L >= 1 && L <= AFM_TURNOVER_MAX_LAGS, "L must be in 1..8");
    AFM_CHECK_ARG(lags, "null buffer (lags)");
    for (int l = 0; l < L; ++l) AFM_CHECK_ARG(lags[l] >= 1, "lags: every lag must be at least 1");
    AFM_CHECK_ARG(base && cols && dates && rows_idx && nrows && rank_ac && counts && port_turn &&
                      scratch, "null buffer");
    AFM_CHECK_ARG(zs || !zcols, "zcols without zs");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(nd < (1ll << 31) && nd * (int64_t)K * L < (1ll << 31),
                  "nd * K * L must be below 2^31");
    if (nd == 0) return AFM_OK;
    const TvLayout y = tv_layout(nd, K, lda);
    const int64_t S = y.slots;
    u64* mk = (u64*)scratch;
    TvMarksArgs ma{base, col_stride, T, lda, cols, K, zs, zcols, dates, 0, 0, 0, S, rows_idx, nrows,
                   y.sort_words ? mk + S * K * y.rec : nullptr, mk};
    TvPairArgs pa{};
    pa.marks = mk;
    pa.lda = lda;
    pa.K = K;
    pa.L = L;
    pa.mod = S;
    pa.rank_ac = rank_ac;
    pa.counts = counts;
    pa.port_turn = port_turn;
    for (int l = 0; l < L; ++l) pa.lag[l] = lags[l];
    {
        const int64_t total = nd * K * L;
        hipLaunchKernelGGL(turnover_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256),
                           0, ctx->stream, pa, total);
        AFM_HIP(hipGetLastError());
    }
    // near lags ride the ring: a block of dates and the largest of them before it stay resident
    const int64_t reach = S >= nd ? nd - 1 : S / 2;
    int64_t near_max = 0;
    unsigned near = 0u;
    for (int l = 0; l < L; ++l) {
        if (lags[l] < nd && lags[l] <= reach) {
            near |= 1u << l;
            if (lags[l] > near_max) near_max = lags[l];
        }
    }
    if (near) {
        const int64_t B = S >= nd ? nd : S - near_max;
        for (int64_t i0 = 0; i0 < nd; i0 += B) {
            const int64_t i1 = i0 + B < nd ? i0 + B : nd;
            int rc = marks(ctx, ma, i0, i1, i0 % S);
            if (rc != AFM_OK) return rc;
            pa.active = near;
            pa.add1 = i0 % S;
            for (int l = 0; l < L; ++l) pa.add0[l] = (((i0 - lags[l]) % S) + S) % S;
            rc = pairs(ctx, pa, i0, i1);
            if (rc != AFM_OK) return rc;
        }
    }
    // a far lag: both sides of a block of pairs computed again, side by side
    for (int l = 0; l < L; ++l) {
        if (lags[l] >= nd || ((near >> l) & 1u)) continue;
        const int64_t lag = lags[l], B = S / 2;
        for (int64_t i0 = lag; i0 < nd; i0 += B) {
            const int64_t i1 = i0 + B < nd ? i0 + B : nd;
            int rc = marks(ctx, ma, i0, i1, 0);
            if (rc != AFM_OK) return rc;
            rc = marks(ctx, ma, i0 - lag, i1 - lag, B);
            if (rc != AFM_OK) return rc;
            pa.active = 1u << l;
            pa.add1 = 0;
            pa.add0[l] = B;
            rc = pairs(ctx, pa, i0, i1);
            if (rc != AFM_OK) return rc;
        }
    }
    return AFM_OK;
}

extern "C" int afm_screen_turnover_summary_f64(afm_ctx* ctx, const double* rank_ac,
                                               const int32_t* counts, const double* port_turn,
                                               int64_t nd, int K, int L, double* stats) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(L >= 1 && L <= AFM_TURNOVER_MAX_LAGS, "L must be in 1..8");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(stats && (nd == 0 || (rank_ac && counts && port_turn)), "null buffer");
    const int64_t tasks = (int64_t)K * L * 4;
    hipLaunchKernelGGL(turnover_summary_kernel, dim3((unsigned)((tasks + 63) / 64)), dim3(64), 0,
                       ctx->stream, nd, K, L, rank_ac, counts, port_turn, stats);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
