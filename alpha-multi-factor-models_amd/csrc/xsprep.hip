// Cross-sectional factor preprocessing (include/afm_xsprep.h): per (date, column) winsorise to
// median +- c MAD or to two quantiles, take out the group means, standardise -- the stage in front
// of the factor screen's kernels, on their row set and their value of a row.
//
//  xsprep_kernel   one workgroup per (date, column), the columns of a date on consecutive
//                  workgroup ids (they share the date's rows_idx and groups in L2).  Phases:
//                    1. gather: the column's values at the date's rows (z-scored on the way when zs
//                       is given, screen_ic_kernel's expression) into register-resident order keys
//                       (screen_layers_kernel's); a missing cell has no key.  A key is its value:
//                       every later phase takes x back out of it.
//                    2. select: the byte-wise radix select of screen_layers_kernel for up to four
//                       ranks at once, by value only (no tie needs a position) -- the two middle
//                       ranks, then the two middle ranks of |x - med| recomputed in registers
//                       (MAD), or the four neighbours of the two quantiles.
//                    3. clip counts, then the sums: group sums of w, the sum of v, the sum of
//                       (v - mu)^2.  Each is formed EXACTLY: the addends are put on a fixed-point
//                       grid chosen from the item's largest magnitude (two 64-bit integer limbs,
//                       92 bits under the largest addend's exponent) and added with integer LDS
//                       atomics, so no order exists that could change a bit.  Means are carried as
//                       double-double and taken out with one rounding.
//                    4. write: the results on the assets of F (a bitmap in LDS records them), NaN
//                       on every other cell of the [lda] row.
//                  Three instantiations by the date's row count as in screen_layers_kernel: up to
//                  kXpFewRows rows kXpFewKeys keys per thread (two workgroups per CU), up to
//                  kXpSelectRows rows kXpSmallKeys, above that kXpLargeKeys.  The row of a key is
//                  j * kXpThreads + tid in all of them.
#include "afm_internal.h"
#include "afm_xsprep.h"

#include <cmath>
#include <vector>

#pragma clang fp contract(off)

#include "afm_np_sum.h"
#include "afm_order.h"                 // okey, unkey, pick_digit

namespace afm {
namespace {

constexpr int kXpThreads = 512;                    // threads per (date, column) workgroup
constexpr int kXpFewKeys = 8;                      // register keys per thread, dates of few rows
constexpr int kXpSmallKeys = 24;                   // ... of more
constexpr int kXpLargeKeys = 64;                   // ... and of many
constexpr int kXpFewRows = 4096;
constexpr int kXpSelectRows = 12288;
constexpr int kXpMaxRows = 32768;                  // lda limit (afm_xs_prepare_f64's)
constexpr int kXpBatch = 8;                        // gathered rows of a thread in flight together
constexpr int kXpTargets = 4;                      // ranks selected together
constexpr int kXpGroups = AFM_XSPREP_MAX_GROUPS;
constexpr int kXpHiBits = 46;                      // bits of the high limb under the largest addend
constexpr int kXpLoBits = 46;                      // bits of the low limb under the high limb's unit
static_assert(kXpFewKeys * kXpThreads == kXpFewRows, "few-key capacity");
static_assert(kXpSmallKeys * kXpThreads == kXpSelectRows, "small capacity");
static_assert(kXpLargeKeys * kXpThreads == kXpMaxRows && kXpLargeKeys <= 64, "large capacity");
static_assert(kXpGroups <= 256 && kXpGroups <= kXpThreads, "a group label is one byte");
// 2^15 addends below 2^(kXpHiBits + 1) (2^kXpLoBits) stay inside a signed 64-bit limb
static_assert(kXpHiBits + 1 + 15 < 63 && kXpLoBits + 1 + 15 < 63, "limbs cannot overflow");

struct XpArgs {
    const double* base;       // plane k: base + cols[k] * col_stride, [T][lda]
    int64_t col_stride, T, lda;
    const int32_t* cols;      // [K]
    int K;
    const double* zs;         // [..][lda][2] {mu, 1/sd}, or null: raw values
    const int32_t* zcols;     // [K] zs row of each column (null: row k)
    const int32_t* dates;     // [nd]
    const int32_t* rows_idx;  // [T][lda]
    const int32_t* nrows;     // [T]
    const int32_t* groups;    // [lda] (g_stride 0) or [T][lda]
    int64_t g_stride;
    int ngroups;
    int winsor;
    double p_lo, p_hi;
    int flags;
    double* out;              // plane k: out + k * out_stride
    int64_t out_stride;
    double* info;             // [nd][K][7]
};

struct XpShared {
    int hist[kXpTargets][256];
    u64 prefix[kXpTargets];
    int need[kXpTargets];
    int nk, nlo, nhi;
    u64 maxbits;                          // the largest |addend| of a sum, as its bit pattern
    i64 acc_hi[kXpGroups], acc_lo[kXpGroups];
    int gcnt[kXpGroups];
    double gmh[kXpGroups], gml[kXpGroups];    // the group means, double-double
    unsigned bitmap[kXpMaxRows / 32];     // assets that have a result
};

// The keys of the 1-based ranks sh.need[q] (0: no such target) among the keyed rows, ascending,
// into sh.prefix[q].  DEV: the rows' keys are those of |x - med|.  Enters and leaves synchronised.
template <int NR, bool DEV>
__device__ __forceinline__ void select(XpShared& sh, const u64 (&ks)[NR], u64 keyed, double med,
                                       int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    u64 pmask = 0ull;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int e = tid; e < kXpTargets * 256; e += kXpThreads) (&sh.hist[0][0])[e] = 0;
        u64 pf[kXpTargets];
        bool act[kXpTargets];
#pragma unroll
        for (int q = 0; q < kXpTargets; ++q) {
            pf[q] = sh.prefix[q];
            act[q] = sh.need[q] > 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if ((keyed >> j) & 1) {
                const u64 kk = DEV ? okey(fabs(unkey(ks[j]) - med)) : ks[j];
                if (shift == 56) {                         // every prefix is empty: one histogram
                    atomicAdd(&sh.hist[0][kk >> 56], 1);
                } else {
#pragma unroll
                    for (int q = 0; q < kXpTargets; ++q)
                        if (act[q] && (kk & pmask) == pf[q])
                            atomicAdd(&sh.hist[q][(kk >> shift) & 255], 1);
                }
            }
        }
        __syncthreads();
        if (wave < kXpTargets) {                           // target q on wave q
            const int q = wave, need = sh.need[q];
            if (need > 0) {
                int d = 0, before = 0;
                if (pick_digit(sh.hist[shift == 56 ? 0 : q], need, lane, d, before)) {
                    sh.prefix[q] |= (u64)d << shift;
                    sh.need[q] = need - before;
                }
            }
        }
        pmask |= 255ull << shift;
        __syncthreads();
    }
}

// ---- exact sums -------------------------------------------------------------------------------
// An addend a with |a| <= M = 2^ex * [1, 2) is a * 2^(kXpHiBits - ex) = hi + lo * 2^-kXpLoBits, hi
// its integer part (|hi| < 2^(kXpHiBits + 1)) and lo the rest rounded to an integer: what is
// dropped is below M * 2^-(kXpHiBits + kXpLoBits).  Integer sums have no order.
struct dd { double h, l; };
__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ void limbs(double a, int sc, i64& hi, i64& lo) {
    const double s = ldexp(a, sc);
    const double th = trunc(s);
    hi = (i64)th;
    lo = (i64)rint(ldexp(s - th, kXpLoBits));
}
// (sum_hi + sum_lo * 2^-kXpLoBits) * 2^-sc as a double-double
__device__ __forceinline__ dd limbs_value(i64 hs, i64 ls, int sc) {
    const double A = ldexp((double)(hs >> 32), 32), B = (double)(hs & 0xffffffffll);
    const double C = ldexp((double)(ls >> 32), 32 - kXpLoBits);
    const double D = ldexp((double)(ls & 0xffffffffll), -kXpLoBits);
    dd s = two_sum(A, B);
    dd t = two_sum(s.h, C);
    double l = s.l + t.l;
    dd u = two_sum(t.h, D);
    l += u.l;
    dd r = two_sum(u.h, l);
    return {ldexp(r.h, -sc), ldexp(r.l, -sc)};
}
__device__ __forceinline__ dd dd_div(dd s, double n) {      // s / n, n a small integer
    const double qh = s.h / n;
    const double r = fma(-qh, n, s.h);
    return {qh, (r + s.l) / n};
}
// a - (m.h + m.l) rounded once: the difference a - m.h exactly (two_sum), then its tail with m.l
__device__ __forceinline__ double minus_dd(double a, double mh, double ml) {
    const dd t = two_sum(a, -mh);
    return t.h + (t.l - ml);
}
__device__ __forceinline__ int scale_of(double M) { return kXpHiBits - ilogb(M); }

// wave-reduced integer add of one slot (all 64 lanes call)
__device__ __forceinline__ void wave_add(i64* slot, i64 v, int lane) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0 && v) atomicAdd(reinterpret_cast<u64*>(slot), (u64)v);
}
__device__ __forceinline__ void wave_max(u64* slot, u64 v, int lane) {
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = __shfl_down(v, o, 64);
        v = w > v ? w : v;
    }
    if (lane == 0 && v) atomicMax(slot, v);
}

// NR: register keys per thread.  The workgroup takes the dates with lo < nrows <= NR * kXpThreads
// (and, for lo < 0, the dates without rows).
template <int NR, bool Z>
__global__ __launch_bounds__(kXpThreads, NR <= kXpFewKeys ? 4 : 2) void xsprep_kernel(XpArgs g,
                                                                                     int lo_rows) {
    __shared__ XpShared sh;
    __shared__ uint8_t sgrp[NR * kXpThreads];              // the group of every keyed row
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t item = blockIdx.x;
    const int64_t di = item / g.K;
    const int k = (int)(item % g.K);
    const int64_t t = g.dates[di];
    if (t < 0 || t >= g.T) return;
    const int lda = (int)g.lda;
    const int n_rows = min(max(g.nrows[t], 0), lda);
    if (n_rows <= lo_rows || n_rows > NR * kXpThreads) return;   // another instantiation's date
    const int64_t base = t * g.lda;
    const double* col = g.base + (int64_t)g.cols[k] * g.col_stride + base;
    const double2* zs2 = Z ? reinterpret_cast<const double2*>(g.zs) +
                                 (int64_t)(g.zcols ? g.zcols[k] : k) * g.lda
                           : nullptr;
    const bool neut = g.flags & AFM_XSPREP_NEUTRALIZE, stdz = g.flags & AFM_XSPREP_STANDARDIZE;
    const int32_t* grp = neut ? g.groups + t * g.g_stride : nullptr;
    double* outrow = g.out + (int64_t)k * g.out_stride + base;
    double* info = g.info + item * AFM_XSPREP_INFO;
    // ---- 1. gather: keys in registers; bit j of `keyed`: row j * kXpThreads + tid has one ------
    u64 ks[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) ks[j] = 0ull;
    u64 keyed = 0ull;
    if (tid == 0) { sh.nk = 0; sh.nlo = 0; sh.nhi = 0; sh.maxbits = 0ull; }
    for (int e = tid; e < kXpMaxRows / 32; e += kXpThreads) sh.bitmap[e] = 0u;
    if (tid < kXpGroups) { sh.acc_hi[tid] = 0; sh.acc_lo[tid] = 0; sh.gcnt[tid] = 0; }
    if (tid < kXpTargets) { sh.prefix[tid] = 0ull; sh.need[tid] = 0; }
    __syncthreads();
    // (batches of kXpBatch rows per thread: the index loads, then the dependent loads, all of a
    // batch in flight together; a thread without a row reads asset 0 instead)
#pragma unroll
    for (int j0 = 0; j0 < NR; j0 += kXpBatch) {
        if (j0 * kXpThreads >= n_rows) break;              // (uniform)
        int a[kXpBatch];
        bool in[kXpBatch];
#pragma unroll
        for (int u = 0; u < kXpBatch; ++u) {
            const int e = (j0 + u) * kXpThreads + tid;
            const int ai = e < n_rows ? g.rows_idx[base + e] : -1;
            in[u] = ai >= 0 && ai < lda;
            a[u] = in[u] ? ai : 0;
        }
        double x[kXpBatch];
        double2 m[Z ? kXpBatch : 1];
        int gi[kXpBatch];
#pragma unroll
        for (int u = 0; u < kXpBatch; ++u) {
            x[u] = col[a[u]];
            if constexpr (Z) m[u] = zs2[a[u]];
            gi[u] = neut ? grp[a[u]] : 0;
        }
#pragma unroll
        for (int u = 0; u < kXpBatch; ++u) {
            const int j = j0 + u;
            double v = x[u];
            if constexpr (Z) v = (v - m[u].x) * m[u].y;    // as the Gram and predict producers
            const bool ok = in[u] && __builtin_isfinite(v) && gi[u] >= 0 && gi[u] < g.ngroups;
            ks[j] = ok ? okey(v) : 0ull;
            keyed |= ok ? 1ull << j : 0ull;
            if (ok) sgrp[j * kXpThreads + tid] = (uint8_t)gi[u];
        }
    }
    {
        int c = __popcll(keyed);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
        if (lane == 0 && c) atomicAdd(&sh.nk, c);
    }
    __syncthreads();
    const int n = sh.nk;
    const double inf = __builtin_huge_val();
    double lo = -inf, hi = inf;
    // ---- 2. select -----------------------------------------------------------------------------
    if (g.winsor != AFM_XSPREP_WINSOR_NONE && n == 0) lo = hi = qnan();
    if (g.winsor == AFM_XSPREP_WINSOR_MAD && n > 0) {
        const int i1 = (n - 1) / 2, i2 = n / 2;            // the middle ranks (0-based)
        if (tid == 0) {
            sh.need[0] = i1 + 1;
            sh.need[1] = i2 != i1 ? i2 + 1 : 0;
        }
        __syncthreads();
        select<NR, false>(sh, ks, keyed, 0.0, tid);
        const double a = unkey(sh.prefix[0]);
        const double med = i2 != i1 ? (a + unkey(sh.prefix[1])) / 2.0 : a;
        __syncthreads();
        if (tid < kXpTargets) {
            sh.prefix[tid] = 0ull;
            sh.need[tid] = tid == 0 ? i1 + 1 : (tid == 1 && i2 != i1 ? i2 + 1 : 0);
        }
        __syncthreads();
        select<NR, true>(sh, ks, keyed, med, tid);
        const double b = unkey(sh.prefix[0]);
        const double mad = i2 != i1 ? (b + unkey(sh.prefix[1])) / 2.0 : b;
        if (mad != 0.0) {
            lo = med - g.p_lo * mad;
            hi = med + g.p_hi * mad;
        }
    } else if (g.winsor == AFM_XSPREP_WINSOR_QUANTILE && n > 0) {
        // numpy's linear quantile: the virtual index (n - 1) q and its two neighbours
        int idx[2];
        double gam[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double v = (double)(n - 1) * (s ? g.p_hi : g.p_lo);
            const double f = floor(v);
            idx[s] = min(max((int)f, 0), n - 1);
            gam[s] = v - f;
        }
        if (tid < kXpTargets) {
            const int i = idx[tid >> 1];
            sh.need[tid] = (tid & 1 ? min(i + 1, n - 1) : i) + 1;
        }
        __syncthreads();
        select<NR, false>(sh, ks, keyed, 0.0, tid);
        double qv[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double a = unkey(sh.prefix[2 * s]), b = unkey(sh.prefix[2 * s + 1]);
            const double diff = b - a;
            qv[s] = gam[s] < 0.5 ? a + diff * gam[s] : b - diff * (1.0 - gam[s]);
        }
        lo = qv[0];
        hi = qv[1];
    }
    // ---- 3. clip counts and sums ---------------------------------------------------------------
    auto clip = [&](double x) { return fmin(fmax(x, lo), hi); };
    {
        int clo = 0, chi = 0;
        u64 mb = 0ull;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if ((keyed >> j) & 1) {
                const double x = unkey(ks[j]);
                clo += x < lo;
                chi += x > hi;
                const u64 b = (u64)__double_as_longlong(fabs(clip(x)));
                mb = b > mb ? b : mb;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            clo += __shfl_down(clo, o, 64);
            chi += __shfl_down(chi, o, 64);
        }
        if (lane == 0 && clo) atomicAdd(&sh.nlo, clo);
        if (lane == 0 && chi) atomicAdd(&sh.nhi, chi);
        if (neut) wave_max(&sh.maxbits, mb, lane);
    }
    __syncthreads();
    if (neut && n > 0) {                                   // group sums of w, exact
        const double M = __longlong_as_double((i64)sh.maxbits);
        const int sc = M > 0.0 ? scale_of(M) : 0;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if ((keyed >> j) & 1) {
                const int gq = sgrp[j * kXpThreads + tid];
                i64 h, l;
                limbs(clip(unkey(ks[j])), sc, h, l);
                atomicAdd(&sh.gcnt[gq], 1);
                if (h) atomicAdd(reinterpret_cast<u64*>(&sh.acc_hi[gq]), (u64)h);
                if (l) atomicAdd(reinterpret_cast<u64*>(&sh.acc_lo[gq]), (u64)l);
            }
        }
        __syncthreads();
        if (tid < kXpGroups) {
            const int c = sh.gcnt[tid];
            dd mean = {0.0, 0.0};
            if (c > 0) mean = dd_div(limbs_value(sh.acc_hi[tid], sh.acc_lo[tid], sc), (double)c);
            sh.gmh[tid] = mean.h;
            sh.gml[tid] = mean.l;
        }
        __syncthreads();
        if (tid < kXpGroups) { sh.acc_hi[tid] = 0; sh.acc_lo[tid] = 0; }
        if (tid == 0) sh.maxbits = 0ull;
    }
    __syncthreads();
    auto value = [&](int j) {                              // v of the keyed row j of this thread
        const double w = clip(unkey(ks[j]));
        if (!neut) return w;
        const int gq = sgrp[j * kXpThreads + tid];
        if (sh.gcnt[gq] == 1) return 0.0;                  // alone in its group: exactly 0
        return minus_dd(w, sh.gmh[gq], sh.gml[gq]);
    };
    // one exact sum over the keyed rows into slot 0: the largest magnitude first, then the limbs
    auto total = [&](auto&& addend, bool& finite) {
        u64 mb = 0ull;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if ((keyed >> j) & 1) {
                const u64 b = (u64)__double_as_longlong(fabs(addend(j)));
                mb = b > mb ? b : mb;
            }
        }
        wave_max(&sh.maxbits, mb, lane);
        __syncthreads();
        const double M = __longlong_as_double((i64)sh.maxbits);
        finite = __builtin_isfinite(M);
        const int sc = finite && M > 0.0 ? scale_of(M) : 0;
        i64 h = 0, l = 0;
        if (finite) {
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                if ((keyed >> j) & 1) {
                    i64 hj, lj;
                    limbs(addend(j), sc, hj, lj);
                    h += hj;
                    l += lj;
                }
            }
        }
        wave_add(&sh.acc_hi[0], h, lane);
        wave_add(&sh.acc_lo[0], l, lane);
        __syncthreads();
        const dd s = limbs_value(sh.acc_hi[0], sh.acc_lo[0], sc);
        __syncthreads();
        if (tid == 0) { sh.acc_hi[0] = 0; sh.acc_lo[0] = 0; sh.maxbits = 0ull; }
        __syncthreads();
        return s;
    };
    double mu_h = 0.0, mu_l = 0.0, mu_out = qnan(), sd = qnan();
    bool good = true;                                      // the item has results
    if (stdz) {
        good = false;
        if (n > 0) {
            bool fin_v = true, fin_d = true;
            const dd sv = total([&](int j) { return value(j); }, fin_v);
            if (fin_v) {
                const dd mu = dd_div(sv, (double)n);
                mu_h = mu.h;
                mu_l = mu.l;
                mu_out = mu.h + mu.l;
                if (n >= 2) {
                    const dd ss = total([&](int j) {
                        const double d = minus_dd(value(j), mu_h, mu_l);
                        return d * d;
                    }, fin_d);
                    if (fin_d) {
                        sd = sqrt((ss.h + ss.l) / (double)(n - 1));
                        good = sd > 0.0 && __builtin_isfinite(sd);
                    }
                }
            }
        }
    }
    // ---- 4. write ------------------------------------------------------------------------------
    if (good) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if ((keyed >> j) & 1) {
                const int a = g.rows_idx[base + j * kXpThreads + tid];   // (in range: it was keyed)
                double r = value(j);
                if (stdz) r = minus_dd(r, mu_h, mu_l) / sd;
                outrow[a] = r;
                atomicOr(&sh.bitmap[a >> 5], 1u << (a & 31));
            }
        }
    }
    __syncthreads();
    for (int a = tid; a < lda; a += kXpThreads)
        if (!((sh.bitmap[a >> 5] >> (a & 31)) & 1u)) outrow[a] = qnan();
    if (tid == 0) {
        info[0] = (double)n;
        info[1] = lo;
        info[2] = hi;
        info[3] = (double)sh.nlo;
        info[4] = (double)sh.nhi;
        info[5] = mu_out;
        info[6] = sd;
    }
}

template <int NR>
void launch_prep(const XpArgs& g, int lo, unsigned grid, hipStream_t stream) {
    if (g.zs)
        hipLaunchKernelGGL((xsprep_kernel<NR, true>), dim3(grid), dim3(kXpThreads), 0, stream, g,
                           lo);
    else
        hipLaunchKernelGGL((xsprep_kernel<NR, false>), dim3(grid), dim3(kXpThreads), 0, stream, g,
                           lo);
}

}  // namespace
}  // namespace afm

using namespace afm;

extern "C" int afm_xs_preprocess_f64(afm_ctx* ctx, const double* base, int64_t col_stride,
                                     int64_t T, int64_t lda, const int32_t* cols, int K,
                                     const double* zs, const int32_t* zcols, const int32_t* dates,
                                     int64_t nd, const int32_t* rows_idx, const int32_t* nrows,
                                     const int32_t* groups, int64_t g_stride, int ngroups,
                                     int winsor, double p_lo, double p_hi, int flags, double* out,
                                     int64_t out_stride, double* info) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(K >= 1, "K must be at least 1");
    AFM_CHECK_ARG(T > 0 && lda > 0 && lda % 64 == 0 && col_stride >= 0,
                  "bad shape (lda a positive multiple of 64)");
    AFM_CHECK_ARG(lda <= kXpMaxRows, "lda must be at most 32768");
    AFM_CHECK_ARG(winsor >= AFM_XSPREP_WINSOR_NONE && winsor <= AFM_XSPREP_WINSOR_QUANTILE,
                  "unknown winsor mode");
    AFM_CHECK_ARG((flags & ~(AFM_XSPREP_NEUTRALIZE | AFM_XSPREP_STANDARDIZE)) == 0,
                  "unknown flag bit");
    if (winsor == AFM_XSPREP_WINSOR_MAD)
        AFM_CHECK_ARG(std::isfinite(p_lo) && std::isfinite(p_hi) && p_lo > 0 && p_hi > 0,
                      "the MAD multiple must be finite and positive");
    if (winsor == AFM_XSPREP_WINSOR_QUANTILE)
        AFM_CHECK_ARG(0 <= p_lo && p_lo < p_hi && p_hi <= 1, "quantiles need 0 <= q_lo < q_hi <= 1");
    if (flags & AFM_XSPREP_NEUTRALIZE) {
        AFM_CHECK_ARG(groups, "neutralisation without groups");
        AFM_CHECK_ARG(ngroups >= 1 && ngroups <= kXpGroups, "ngroups must be in 1..256");
        AFM_CHECK_ARG(g_stride == 0 || g_stride == lda, "g_stride must be 0 or lda");
    }
    AFM_CHECK_ARG(base && cols && dates && rows_idx && nrows && out && info, "null buffer");
    AFM_CHECK_ARG(zs || !zcols, "zcols without zs");
    AFM_CHECK_ARG(out_stride >= T * lda || K == 1, "out_stride is shorter than a plane");
    AFM_CHECK_ARG(nd >= 0, "nd is negative");
    AFM_CHECK_ARG(nd < (1ll << 31) && nd * K < (1ll << 31), "nd * K must be below 2^31");
    if (nd == 0) return AFM_OK;
    {   // out against the planes the call reads (cols comes to the host for it)
        std::vector<int32_t> hc((size_t)K);
        AFM_HIP(hipMemcpyAsync(hc.data(), cols, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost,
                               ctx->stream));
        AFM_HIP(hipStreamSynchronize(ctx->stream));
        const int64_t plane = T * lda;
        const double* o0 = out;
        const double* o1 = out + (int64_t)(K - 1) * out_stride + plane;
        for (int k = 0; k < K; ++k) {
            AFM_CHECK_ARG(hc[(size_t)k] >= 0, "negative column");
            const double* p0 = base + (int64_t)hc[(size_t)k] * col_stride;
            AFM_CHECK_ARG(p0 + plane <= o0 || o1 <= p0, "out overlaps a plane it reads");
        }
    }
    XpArgs g{base, col_stride, T, lda, cols, K, zs, zcols, dates, rows_idx, nrows, groups,
             g_stride, (flags & AFM_XSPREP_NEUTRALIZE) ? ngroups : 1, winsor, p_lo, p_hi, flags,
             out, out_stride, info};
    const int64_t items = nd * K;
    launch_prep<kXpFewKeys>(g, -1, (unsigned)items, ctx->stream);
    AFM_HIP(hipGetLastError());
    if (lda > kXpFewRows) {
        launch_prep<kXpSmallKeys>(g, kXpFewRows, (unsigned)items, ctx->stream);
        AFM_HIP(hipGetLastError());
    }
    if (lda > kXpSelectRows) {
        launch_prep<kXpLargeKeys>(g, kXpSelectRows, (unsigned)items, ctx->stream);
        AFM_HIP(hipGetLastError());
    }
    return AFM_OK;
}
