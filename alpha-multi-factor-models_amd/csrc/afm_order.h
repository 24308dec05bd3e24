// The ordering primitives of the cross-sectional rank kernels, one copy each: the order key of a
// double, the decile layer of a rank, the run sort with its bound search, the digit pick of a
// radix select and the ten-target decile select.  Device code only (pow2_at_least also sizes the
// launchers' LDS).  The results of its users must round exactly like pandas / numpy: the
// translation units are built with -ffp-contract=off and set `#pragma clang fp contract(off)`
// before including this header.
#pragma once
#include <hip/hip_runtime.h>

namespace afm {
namespace {

typedef unsigned long long u64;
typedef long long i64;

// ---- keys ----------------------------------------------------------------------------------------
__device__ __forceinline__ u64 okey(double v) {    // order-preserving key, -0.0 == +0.0
    if (v == 0.0) v = 0.0;
    u64 u = (u64)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double unkey(u64 k) {   // the value of a key
    const u64 u = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
    return __longlong_as_double((i64)u);
}

constexpr int kOrdLayers = 10;
__device__ __forceinline__ int layer_of(int r, int n) {   // KKT:328-330
    int l = (int)((double)r / (double)n * kOrdLayers) + 1;
    return l > kOrdLayers ? kOrdLayers : l;
}

// ---- run sort --------------------------------------------------------------------------------------
// The rows of a date are sorted in runs, each a bitonic network in LDS over a power of two: runs
// of kSortChunk rows while that many are left, then the largest power of two that fits while at
// least 2 * kSortMinRun rows are left, then the rest padded.  A date of up to kSortLdsRows rows
// keeps its runs side by side in LDS; a longer one writes each sorted run to the workgroup's
// scratch.  A key's bounds among all rows are the sums of its bounds in every run.
constexpr int kSortThreads = 1024;     // the workgroup of every caller (16 waves)
constexpr int kSortLdsRows = 16384;    // rows of a date sorted and searched in LDS (128 KB of keys)
constexpr int kSortChunk = 16384;      // rows of the longest sorted run
constexpr int kSortMinRun = 1024;      // no run is split below twice this
constexpr u64 kSortPad = ~0ull;        // above the key of every finite value and of +-inf
static_assert(kSortChunk == kSortLdsRows && (kSortChunk & (kSortChunk - 1)) == 0 &&
              kSortChunk % (2 * kSortMinRun) == 0, "runs sort in LDS, side by side");

__host__ __device__ __forceinline__ int pow2_at_least(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// ascending bitonic sort of key[0, P), P a power of two; ends with a barrier
__device__ void bitonic_sort(u64* key, int P) {
    const int tid = threadIdx.x;
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = tid; e < P / 2; e += kSortThreads) {
                const int lo = 2 * e - (e & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const u64 ka = key[lo], kb = key[hi];
                if ((ka > kb) == up && ka != kb) {
                    key[lo] = kb;
                    key[hi] = ka;
                }
            }
            __syncthreads();
        }
    }
}

// rows of the next sorted run when rem > 0 rows are left (a power of two unless it is the last)
__device__ __forceinline__ int run_rows(int rem) {
    if (rem >= kSortChunk) return kSortChunk;
    return rem >= 2 * kSortMinRun ? 1 << (31 - __clz(rem)) : rem;
}

// The keys keyfn(e), e in [0, n), sorted run by run: run [c0, c0 + len) at lds + c0 when n <=
// kSortLdsRows (only the last run is padded, so the runs do not overlap), else at scr + c0.  All
// threads call it; it opens with a barrier (the previous searches are done) and LDS and scr hold
// the result after the closing one.
template <class KeyFn>
__device__ void sort_rows(u64* lds, u64* scr, int n, KeyFn keyfn) {
    const int tid = threadIdx.x;
    const bool in_lds = n <= kSortLdsRows;
    __syncthreads();
    for (int c0 = 0; c0 < n;) {
        const int len = run_rows(n - c0);
        const int P = pow2_at_least(len);
        u64* buf = in_lds ? lds + c0 : lds;
        for (int e = tid; e < P; e += kSortThreads) buf[e] = e < len ? keyfn(c0 + e) : kSortPad;
        __syncthreads();
        bitonic_sort(buf, P);
        if (!in_lds) {
            for (int e = tid; e < len; e += kSortThreads) scr[c0 + e] = buf[e];
            __syncthreads();
        }
        c0 += len;
    }
}

// lb += the keys of the sorted run K[0, len) below k, ub += those up to k
template <class Ptr>
__device__ __forceinline__ void run_bounds(Ptr K, int len, u64 k, int& lb, int& ub) {
    int lo = 0, hi = len;
    while (lo < hi) {                                      // first key >= k
        const int m = (lo + hi) >> 1;
        if (K[m] < k) lo = m + 1; else hi = m;
    }
    lb += lo;
    hi = len;
    while (lo < hi) {                                      // first key > k
        const int m = (lo + hi) >> 1;
        if (K[m] <= k) lo = m + 1; else hi = m;
    }
    ub += lo;
}

// The rows of sort_rows' result with a key below k (lb) and up to k (ub): 2 * (average rank) of
// a row's own key is 1 + lb + ub.  One loop per memory, so that the LDS searches read LDS.
__device__ __forceinline__ void bounds(const u64* lds, const u64* scr, int n, u64 k, int& lb,
                                       int& ub) {
    lb = 0;
    ub = 0;
    if (n <= kSortLdsRows) {
        for (int c0 = 0; c0 < n;) {
            const int len = run_rows(n - c0);
            run_bounds(lds + c0, len, k, lb, ub);
            c0 += len;
        }
    } else {
        for (int c0 = 0; c0 < n;) {
            const int len = run_rows(n - c0);
            run_bounds(scr + c0, len, k, lb, ub);
            c0 += len;
        }
    }
}

// ---- digit pick ------------------------------------------------------------------------------------
// The smallest digit d of a 256-bin histogram whose cumulative count reaches `need`, by one wave
// (bins 4 * lane .. 4 * lane + 3 per lane).  True on the lane that holds d; `before` = the count
// of the smaller digits.
__device__ __forceinline__ bool pick_digit(const int* h, int need, int lane, int& d, int& before) {
    const int h0 = h[4 * lane], h1 = h[4 * lane + 1], h2 = h[4 * lane + 2], h3 = h[4 * lane + 3];
    const int s4 = h0 + h1 + h2 + h3;
    int P = s4;                                            // inclusive prefix over lanes
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(P, o, 64);
        if (lane >= o) P += v;
    }
    const u64 m = __ballot(P >= need);
    if (!m || lane != __builtin_ctzll(m)) return false;
    int acc = P - s4;
    if (acc + h0 >= need) { d = 4 * lane; }
    else if (acc + h0 + h1 >= need) { d = 4 * lane + 1; acc += h0; }
    else if (acc + h0 + h1 + h2 >= need) { d = 4 * lane + 2; acc += h0 + h1; }
    else { d = 4 * lane + 3; acc += h0 + h1 + h2; }
    before = acc;
    return true;
}

// ---- decile select ---------------------------------------------------------------------------------
// A row's layer is monotone in its rank, so with R_l = the largest rank of layer <= l, layer(e) =
// 1 + #{l < 10 : (key_e, e) > the R_l-th smallest (key, position)}: nine order statistics, found
// by one radix select that narrows all nine prefixes in the same passes over register-resident
// keys, exact ties resolved by position.  The 10th largest (key descending, position ascending)
// is a tenth target of the same select, on the complemented key.
constexpr int kSelTargets = 10;           // 9 decile bounds + the 10th largest
constexpr int kSelTop = 10;

struct DecileSelect {
    int hist[kSelTargets][256];
    u64 prefix[kSelTargets];              // the target row's key (complemented for the last)
    int need[kSelTargets];
    int rneed[kSelTargets];               // target rank (1-based), 0 = no row
    int eqidx[kSelTargets];               // the position of the target row
};

// NR register keys per thread of an NT-thread workgroup: row j * NT + tid has the key ks[j] when
// bit j of `keyed` is set, nk > 0 keyed rows in all.  Positions are selected in two passes of TB
// bits.  All threads call it; it leaves prefix, eqidx and rneed in sh, synchronised.
template <int NR, int NT, int TB>
__device__ __forceinline__ void decile_select(DecileSelect& sh, const u64 (&ks)[NR], u64 keyed,
                                              int nk, int tid) {
    static_assert(NR <= 64 && NR * NT <= 1 << (2 * TB) && TB <= 8, "positions fit two tie passes");
    const int lane = tid & 63, wave = tid >> 6;
    if (tid < kSelTargets) {
        int r;
        if (tid < kSelTargets - 1) {      // R_l: the largest rank with layer <= l (l = tid + 1)
            int lo = 0, hi = nk;          // f(lo) <= l (f(0) := 0), f(hi + 1) > l or hi = nk
            while (lo < hi) {
                const int m = (lo + hi + 1) >> 1;
                if (layer_of(m, nk) <= tid + 1) lo = m; else hi = m - 1;
            }
            r = lo;
        } else {
            r = nk >= kSelTop ? kSelTop : nk;              // the 10th largest (or the n_k-th)
        }
        sh.rneed[tid] = r;
        sh.need[tid] = r;
        sh.prefix[tid] = 0ull;
        sh.eqidx[tid] = 0;
    }
    __syncthreads();
    u64 pmask = 0ull;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int e = tid; e < kSelTargets * 256; e += NT) (&sh.hist[0][0])[e] = 0;
        __syncthreads();
        if (shift == 56) {
            // every target's prefix is empty: one histogram of the top digit, copied to the
            // ascending targets and mirrored for the complemented one
#pragma unroll
            for (int j = 0; j < NR; ++j)
                if ((keyed >> j) & 1) atomicAdd(&sh.hist[0][ks[j] >> 56], 1);
            __syncthreads();
            if (tid < 256) {
                const int h = sh.hist[0][tid];
#pragma unroll
                for (int q = 1; q < kSelTargets - 1; ++q) sh.hist[q][tid] = h;
                sh.hist[kSelTargets - 1][255 - tid] = h;
            }
        } else {
            u64 pf[kSelTargets];
            bool act[kSelTargets];
#pragma unroll
            for (int q = 0; q < kSelTargets; ++q) {
                pf[q] = sh.prefix[q];
                act[q] = sh.need[q] > 0;
            }
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                if ((keyed >> j) & 1) {
#pragma unroll
                    for (int q = 0; q < kSelTargets; ++q) {
                        const u64 kk = q < kSelTargets - 1 ? ks[j] : ~ks[j];
                        if (act[q] && (kk & pmask) == pf[q])
                            atomicAdd(&sh.hist[q][(kk >> shift) & 255], 1);
                    }
                }
            }
        }
        __syncthreads();
        for (int q = wave; q < kSelTargets; q += NT / 64) {    // target q on wave q % (NT / 64)
            const int need = sh.need[q];
            if (need > 0) {
                int d = 0, before = 0;
                if (pick_digit(sh.hist[q], need, lane, d, before)) {
                    sh.prefix[q] |= (u64)d << shift;
                    sh.need[q] = need - before;
                }
            }
        }
        pmask |= 255ull << shift;
        __syncthreads();
    }
    // ties at each target's key: the need-th smallest position among them, by the same select
    // over the positions (two passes of TB bits)
    constexpr int kDigit = (1 << TB) - 1;
    int epfx[kSelTargets];
#pragma unroll
    for (int q = 0; q < kSelTargets; ++q) epfx[q] = 0;
    int emask = 0;
    for (int shift = TB; shift >= 0; shift -= TB) {
        for (int e = tid; e < kSelTargets * 256; e += NT) (&sh.hist[0][0])[e] = 0;
        u64 pf[kSelTargets];
        bool act[kSelTargets];
#pragma unroll
        for (int q = 0; q < kSelTargets; ++q) {
            pf[q] = sh.prefix[q];
            act[q] = sh.need[q] > 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int e = j * NT + tid;
            if ((keyed >> j) & 1) {
#pragma unroll
                for (int q = 0; q < kSelTargets; ++q) {
                    const u64 kk = q < kSelTargets - 1 ? ks[j] : ~ks[j];
                    if (act[q] && kk == pf[q] && (e & emask) == epfx[q])
                        atomicAdd(&sh.hist[q][(e >> shift) & kDigit], 1);
                }
            }
        }
        __syncthreads();
        for (int q = wave; q < kSelTargets; q += NT / 64) {
            const int need = sh.need[q];
            if (need > 0) {
                int d = 0, before = 0;
                if (pick_digit(sh.hist[q], need, lane, d, before)) {
                    sh.eqidx[q] = (shift == TB ? 0 : sh.eqidx[q]) | (d << shift);
                    sh.need[q] = need - before;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kSelTargets; ++q) epfx[q] = sh.need[q] > 0 ? sh.eqidx[q] : 0;
        emask |= kDigit << shift;
        __syncthreads();
    }
}

}  // namespace
}  // namespace afm
