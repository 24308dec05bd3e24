// numpy's summation order in device code, shared by analyzer.hip and screen.hip: the results of
// both must round exactly like pandas / numpy (the translation units are built with
// -ffp-contract=off and set `#pragma clang fp contract(off)` before including this header).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace afm {
namespace {

__device__ __forceinline__ double qnan() { return __builtin_nan(""); }

// one leaf of numpy's pairwise_sum: n <= 128 values (the 8-accumulator block, or the plain loop
// under 8)
__device__ double leaf_sum(const double* a, int n) {
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i;
    for (i = 8; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// np.add.reduce of v[0..n) is the identity 0.0, then numpy's pairwise sums of the consecutive
// kNpBuf-element buffers of the ufunc's buffered reduction added one by one (over 8192 elements
// the sum is not one pairwise tree: oracle np_sum, pinned to numpy in tests/test_oracle_golden.py)
constexpr int64_t kNpBuf = 8192;

__device__ double seq_pairwise(const double* a, int64_t n) {   // numpy pairwise_sum, one thread
    if (n <= 128) return leaf_sum(a, (int)n);
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return seq_pairwise(a, n2) + seq_pairwise(a + n2, n - n2);
}
__device__ double seq_np_sum(const double* a, int64_t n) {      // np.add.reduce, one thread
    double r = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += kNpBuf) r = r + seq_pairwise(a + c0, n - c0 < kNpBuf ? n - c0 : kNpBuf);
    return r;
}

// The same sums of a sequence that is not contiguous in memory: element i is get(i0 + i) (a
// strided view, a value mapped on the way).  Operation for operation leaf_sum / seq_pairwise /
// seq_np_sum above.
template <class Get>
__device__ double leaf_sum_of(Get get, int64_t i0, int n) {
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; ++i) res += get(i0 + i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = get(i0 + j);
    int i;
    for (i = 8; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += get(i0 + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += get(i0 + i);
    return res;
}
template <class Get>
__device__ double seq_pairwise_of(Get get, int64_t i0, int64_t n) {
    if (n <= 128) return leaf_sum_of(get, i0, (int)n);
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return seq_pairwise_of(get, i0, n2) + seq_pairwise_of(get, i0 + n2, n - n2);
}
template <class Get>
__device__ double seq_np_sum_of(Get get, int64_t n) {
    double r = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += kNpBuf)
        r = r + seq_pairwise_of(get, c0, n - c0 < kNpBuf ? n - c0 : kNpBuf);
    return r;
}

}  // namespace
}  // namespace afm
