// The factor risk model of include/afm_risk.h: residuals of the per-date regressions, the EWMA
// factor covariance (West's update), the EWMA specific variance with its cross-sectional fill, and
// the covariance B F B' + D and risk decomposition of the rebalance books.  The header pins every
// order of addition; tests/risk_ref.py restates it in numpy and the kernels equal it bit for bit
// (fp contraction off: one IEEE operation per operator).
//
// risk_resid_kernel    -- one thread per (date, security): p exposure planes and the label plane
//                         read once, coalesced along the securities; the date's coefficients and
//                         column offsets in LDS.
// risk_fcov_kernel     -- one workgroup: thread e owns up to 3 of the K1 (K1 + 1) / 2 pairs i >= j
//                         of C in registers; the dates are sequential, the rows of beta staged
//                         through LDS 64 dates at a time, one barrier per used date.
// risk_spec_kernel     -- one lane per security walking its column in date order, 16 loads ahead.
// risk_fill_kernel     -- one workgroup per date: the finite values compacted in order into LDS
//                         runs of 8192, each summed as numpy's pairwise tree.
// risk_book_kernel     -- one workgroup per (date, side) and one for the net book: B, F and G in
//                         LDS (rows padded to 33: the pair loops read two rows at unit stride).
#include "afm_internal.h"
#include "afm_risk.h"

#include <cmath>

#pragma clang fp contract(off)

#include "afm_np_sum.h"                // seq_pairwise, qnan

namespace afm {
namespace {

constexpr int kMaxF = AFM_RISK_MAX_FACTORS;    // K1 cap
constexpr int kFs = kMaxF + 1;                 // padded row stride of the factor matrices in LDS
constexpr int kBook = AFM_MAX_BOOK;
constexpr int kRun = 8192;                     // np.add.reduce's buffer

// row-major lower-triangle pair e -> (i >= j)
__device__ __forceinline__ void pair_of(int e, int& i, int& j) {
    int a = (int)((__builtin_sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    if (a * (a + 1) / 2 > e) --a;
    if ((a + 1) * (a + 2) / 2 <= e) ++a;
    i = a;
    j = e - a * (a + 1) / 2;
}

// the date is used: no regressor dropped, every coefficient finite
__device__ __forceinline__ bool date_used(const double* b, int K1, int rank) {
    bool u = rank == K1 - 1;
    for (int c = 0; c < K1; ++c) u = u && __builtin_isfinite(b[c]);
    return u;
}

__global__ __launch_bounds__(256) void risk_resid_kernel(const double* base, int64_t col_stride,
                                                         int64_t A, int64_t lda,
                                                         const int32_t* cols, int p, int ycol,
                                                         const double* beta, const int32_t* rank,
                                                         const uint64_t* bits, double* resid) {
    __shared__ double sb[kMaxF];
    __shared__ int64_t so[kMaxF];
    __shared__ int sused;
    const int tid = threadIdx.x, K1 = p + 1;
    const int64_t nb = (lda + 255) / 256;
    const int64_t t = blockIdx.x / nb, a = (blockIdx.x % nb) * 256 + tid;
    if (tid < K1) {
        sb[tid] = beta[t * K1 + tid];
        so[tid] = tid ? (int64_t)cols[tid - 1] * col_stride : 0;
    }
    __syncthreads();
    if (tid == 0) sused = date_used(sb, K1, rank[t]) ? 1 : 0;
    __syncthreads();
    if (a >= lda) return;
    double u = qnan();
    if (sused && a < A && ((bits[(t >> 6) * lda + a] >> (t & 63)) & 1ull)) {
        const double* cell = base + t * lda + a;
        const double y = cell[(int64_t)ycol * col_stride];
        bool fin = __builtin_isfinite(y);
        double acc = sb[0];
        for (int j0 = 1; j0 < K1; j0 += 8) {           // 8 plane loads in flight, added in order
            double x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = j0 + q < K1 ? cell[so[j0 + q]] : 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (j0 + q < K1) {
                    fin = fin && __builtin_isfinite(x[q]);
                    acc = acc + sb[j0 + q] * x[q];
                }
            }
        }
        if (fin) u = y - acc;
    }
    resid[t * lda + a] = u;
}

__global__ __launch_bounds__(256) void risk_fcov_kernel(const double* beta, const int32_t* rank,
                                                        int64_t T, int p, double lam, int min_obs,
                                                        int lag, double* fcov, int32_t* nused) {
    __shared__ double fs[64][kFs];
    __shared__ double sd[2][kMaxF];
    __shared__ int su[64];
    const int tid = threadIdx.x, K1 = p + 1, np = K1 * (K1 + 1) / 2, KK = K1 * K1;
    constexpr int EPT = (kMaxF * (kMaxF + 1) / 2 + 255) / 256;
    int pi[EPT], pj[EPT];
    double C[EPT];
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
        pair_of(tid + 256 * m, pi[m], pj[m]);
        C[m] = 0.0;
    }
    // the dates before the first state is due
    const int64_t head = lag < T ? lag : T;
    for (int64_t e = tid; e < head * KK; e += 256) fcov[e] = qnan();
    for (int64_t e = tid; e < head; e += 256) nused[e] = 0;
    double W = 0.0, mean = 0.0;                        // mean: m_tid of the threads below K1
    int cnt = 0, buf = 0;
    for (int64_t c0 = 0; c0 < T; c0 += 64) {
        const int nr = (int)(T - c0 < 64 ? T - c0 : 64);
        __syncthreads();                               // the previous chunk is read
        for (int e = tid; e < nr * K1; e += 256) fs[e / K1][e % K1] = beta[c0 * K1 + e];
        __syncthreads();
        if (tid < nr) su[tid] = date_used(fs[tid], K1, rank[c0 + tid]) ? 1 : 0;
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            if (su[r]) {                               // uniform
                const double lw = lam * W;
                const double Wn = lw + 1.0;
                const double g = lw / Wn;
                if (tid < K1) {
                    const double d = fs[r][tid] - mean;
                    mean = mean + d / Wn;
                    sd[buf][tid] = d;
                }
                __syncthreads();
#pragma unroll
                for (int m = 0; m < EPT; ++m)
                    if (tid + 256 * m < np) C[m] = lam * C[m] + (g * sd[buf][pi[m]]) * sd[buf][pj[m]];
                buf ^= 1;                              // the next used date writes the other copy
                W = Wn;
                ++cnt;
            }
            const int64_t to = c0 + r + lag;
            if (to < T) {
                double* out = fcov + to * KK;
                const bool ok = cnt >= min_obs;
#pragma unroll
                for (int m = 0; m < EPT; ++m) {
                    if (tid + 256 * m < np) {
                        const double v = ok ? C[m] / W : qnan();
                        out[pi[m] * K1 + pj[m]] = v;
                        out[pj[m] * K1 + pi[m]] = v;
                    }
                }
                if (tid == 0) nused[to] = cnt;
            }
        }
    }
}

__global__ __launch_bounds__(64) void risk_spec_kernel(const double* resid, int64_t T, int64_t A,
                                                       int64_t lda, double lam, int min_obs,
                                                       int lag, double* spec) {
    const int64_t a = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (a >= lda) return;
    const bool col = a < A;
    const int64_t head = lag < T ? lag : T;
    for (int64_t t = 0; t < head; ++t) spec[t * lda + a] = qnan();
    double W = 0.0, D = 0.0;
    int n = 0;
    constexpr int PF = 16;
    for (int64_t s0 = 0; s0 < T; s0 += PF) {
        double u[PF];
#pragma unroll
        for (int q = 0; q < PF; ++q) u[q] = col && s0 + q < T ? resid[(s0 + q) * lda + a] : qnan();
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            const int64_t s = s0 + q;
            if (s < T) {
                if (__builtin_isfinite(u[q])) {
                    W = lam * W + 1.0;
                    D = lam * D + u[q] * u[q];
                    ++n;
                }
                if (s + lag < T) spec[(s + lag) * lda + a] = col && n >= min_obs ? D / W : qnan();
            }
        }
    }
}

// dynamic LDS: kRun + 256 doubles
__global__ __launch_bounds__(256) void risk_fill_kernel(const double* spec, int64_t A, int64_t lda,
                                                        double* fill) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* run = reinterpret_cast<double*>(smem_raw);
    __shared__ int wc[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double* row = spec + (int64_t)blockIdx.x * lda;
    int cnt = 0;                                       // uniform: values waiting in run
    int64_t total = 0;
    double r = 0.0;                                    // thread 0: np.add.reduce's accumulator
    for (int64_t a0 = 0; a0 < A; a0 += 256) {
        const int64_t a = a0 + tid;
        const double v = a < A ? row[a] : qnan();
        const bool f = __builtin_isfinite(v);
        const unsigned long long m = __ballot(f);
        if (lane == 0) wc[wv] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            off += w < wv ? wc[w] : 0;
            tot += wc[w];
        }
        if (f) run[cnt + off + __popcll(m & ((1ull << lane) - 1ull))] = v;   // < kRun + 256
        cnt += tot;
        __syncthreads();
        if (cnt >= kRun) {
            if (tid == 0) r = r + seq_pairwise(run, kRun);
            const int rest = cnt - kRun;               // < 256
            const double mv = tid < rest ? run[kRun + tid] : 0.0;
            __syncthreads();
            if (tid < rest) run[tid] = mv;
            cnt = rest;
            total += kRun;
            __syncthreads();
        }
    }
    if (tid == 0) {
        if (cnt > 0) r = r + seq_pairwise(run, cnt);
        total += cnt;
        fill[blockIdx.x] = total > 0 ? r / (double)total : qnan();
    }
}

struct BookArgs {
    const double* base;
    int64_t col_stride, T, lda;
    const int32_t* cols;
    int p;
    const int32_t* dates;
    const int32_t* k;
    const int32_t* books;      // [nd][2][kBook]
    const double* weights;     // [nd][2][kBook]
    const double* fcov;        // [T][K1][K1]
    const double* spec;        // [T][lda]
    const double* fill;        // [T]
    int kc;
    double* cov;               // [nd][2][kc][kc]
    double* risk;              // [nd][3][4]
    double* contrib;           // [nd][3][K1]
    int32_t* status;           // [nd], zeroed by the launcher
};

struct BookLds {
    double B[kBook][kFs];      // exposures of (a chunk of) the members
    double G[kBook][kFs];      // B F
    double F[kMaxF][kFs];
    double w[2 * kBook], d[2 * kBook];
    double x[kMaxF], c[kMaxF];
    int mem[2 * kBook];
    int bl[kBook], bs[kBook], fresh[kBook];
    int64_t off[kMaxF];        // plane offsets of the factors (off[0] unused)
    int n, filled;
};

static_assert(sizeof(BookLds) <= 96 * 1024, "book risk LDS");

__global__ __launch_bounds__(256) void risk_book_kernel(BookArgs r) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    BookLds& sh = *reinterpret_cast<BookLds*>(smem_raw);
    const int tid = threadIdx.x, K1 = r.p + 1;
    const int64_t i = blockIdx.x;
    const int side = blockIdx.y;                       // 0 long, 1 short, 2 net
    const int k = r.k[i];
    if (k < 0 || k > r.kc) {                           // uniform
        if (tid == 0 && side == 0) atomicOr(&r.status[i], 2);
        return;
    }
    const int64_t t = r.dates[i];
    int bad = t < 0 || t >= r.T;
    // ---- F, the member list and its weights ------------------------------------------------------
    if (!bad) {
        for (int e = tid; e < K1 * K1; e += 256) {
            const double v = r.fcov[t * K1 * K1 + e];
            sh.F[e / K1][e % K1] = v;
            bad |= !__builtin_isfinite(v);
        }
    }
    if (tid < K1) sh.off[tid] = tid ? (int64_t)r.cols[tid - 1] * r.col_stride : 0;
    if (tid == 0) sh.filled = 0;
    const int32_t* bL = r.books + (i * 2) * kBook;
    const double* wL = r.weights + (i * 2) * kBook;
    if (side < 2) {
        if (tid < k) {
            sh.mem[tid] = bL[side * kBook + tid];
            sh.w[tid] = wL[side * kBook + tid];
        }
        if (tid == 0) sh.n = k;
        __syncthreads();
    } else {
        if (tid < k) {
            sh.bl[tid] = bL[tid];
            sh.bs[tid] = bL[kBook + tid];
        }
        __syncthreads();
        if (tid < k) {
            double ws = 0.0;
            int inl = 0;
            for (int q = 0; q < k; ++q) {
                if (sh.bs[q] == sh.bl[tid]) ws = wL[kBook + q];
                inl |= sh.bl[q] == sh.bs[tid];
            }
            sh.mem[tid] = sh.bl[tid];
            sh.w[tid] = (wL[tid] - ws) / 2.0;
            sh.fresh[tid] = !inl;
        }
        __syncthreads();
        if (tid == 0) {
            int n = k;
            for (int q = 0; q < k; ++q) {
                if (sh.fresh[q]) {
                    sh.mem[n] = sh.bs[q];
                    sh.w[n] = (0.0 - wL[kBook + q]) / 2.0;
                    ++n;
                }
            }
            sh.n = n;
        }
        __syncthreads();
    }
    const int n = sh.n;
    // ---- d_m: the specific variance, or the date's fill ---------------------------------------------
    if (!bad) {
        const double fv = r.fill[t];
        for (int m = tid; m < n; m += 256) {
            const int a = sh.mem[m];
            double v = qnan();
            if (a < 0 || a >= r.lda) {
                bad = 1;
            } else {
                v = r.spec[t * r.lda + a];
                if (!__builtin_isfinite(v)) {
                    v = fv;
                    atomicAdd(&sh.filled, 1);
                    bad |= !__builtin_isfinite(fv);
                }
            }
            sh.d[m] = v;
        }
    }
    double* risk = r.risk + (i * 3 + side) * 4;
    double* contrib = r.contrib + (i * 3 + side) * K1;
    double* cov = side < 2 ? r.cov + (i * 2 + side) * (int64_t)r.kc * r.kc : nullptr;
    if (__syncthreads_or(bad)) {
        if (tid < 4) risk[tid] = qnan();
        if (tid < K1) contrib[tid] = qnan();
        if (side < 2)
            for (int e = tid; e < k * k; e += 256) cov[(e / k) * r.kc + e % k] = qnan();
        if (tid == 0) atomicOr(&r.status[i], 4);
        return;
    }
    // ---- x = B'w, the members' exposures staged 128 at a time ---------------------------------------
    double x = 0.0;
    for (int c0 = 0; c0 < n; c0 += kBook) {
        const int cn = n - c0 < kBook ? n - c0 : kBook;
        if (c0) __syncthreads();
        for (int e = tid; e < cn * K1; e += 256) {
            const int f = e / cn, mm = e - f * cn;         // members fastest: one plane per pass
            double v = 1.0;
            if (f) {
                v = r.base[sh.off[f] + t * r.lda + sh.mem[c0 + mm]];
                v = __builtin_isfinite(v) ? v : 0.0;
            }
            sh.B[mm][f] = v;
        }
        __syncthreads();
        if (tid < K1)
            for (int mm = 0; mm < cn; ++mm) x = x + sh.B[mm][tid] * sh.w[c0 + mm];
    }
    if (tid < K1) sh.x[tid] = x;
    __syncthreads();
    if (tid < K1) {
        double fx = 0.0;
        for (int j = 0; j < K1; ++j) fx = fx + sh.F[tid][j] * sh.x[j];
        const double c = sh.x[tid] * fx;
        sh.c[tid] = c;
        contrib[tid] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double fvar = 0.0, svar = 0.0;
        for (int f = 0; f < K1; ++f) fvar = fvar + sh.c[f];
        for (int m = 0; m < n; ++m) svar = svar + (sh.w[m] * sh.w[m]) * sh.d[m];
        risk[0] = fvar + svar;
        risk[1] = fvar;
        risk[2] = svar;
        risk[3] = (double)sh.filled;
    }
    if (side == 2) return;
    // ---- G = B F, S = G B' + D (one chunk: n = k <= 128 members) -------------------------------------
    for (int e = tid; e < k * K1; e += 256) {
        const int m = e / K1, j = e - m * K1;
        double acc = 0.0;
        for (int f = 0; f < K1; ++f) acc = acc + sh.B[m][f] * sh.F[f][j];
        sh.G[m][j] = acc;
    }
    __syncthreads();
    for (int e = tid; e < k * (k + 1) / 2; e += 256) {
        int m, q;
        pair_of(e, m, q);
        double acc = 0.0;
        for (int j = 0; j < K1; ++j) acc = acc + sh.G[m][j] * sh.B[q][j];
        if (m == q) acc = acc + sh.d[m];
        cov[(int64_t)m * r.kc + q] = acc;
        cov[(int64_t)q * r.kc + m] = acc;
    }
}

}  // namespace
}  // namespace afm

using namespace afm;

static bool risk_shape_ok(int64_t T, int64_t A, int64_t lda) {
    return T >= 1 && A >= 1 && lda >= A && lda % 64 == 0;
}

extern "C" int afm_risk_resid_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                                  int64_t A, int64_t lda, const int32_t* cols, int p, int ycol,
                                  const double* beta, const int32_t* rank, const uint64_t* bits,
                                  double* resid) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(p >= 1 && p < kMaxF, "need 1 <= p and p + 1 <= AFM_RISK_MAX_FACTORS");
    AFM_CHECK_ARG(risk_shape_ok(T, A, lda), "bad panel shape");
    AFM_CHECK_ARG(base && cols && beta && rank && bits && resid && ycol >= 0, "null buffer");
    const int64_t nb = (lda + 255) / 256;
    AFM_CHECK_ARG(T * nb < ((int64_t)1 << 31), "T x lda too large for one launch");
    hipLaunchKernelGGL(risk_resid_kernel, dim3((unsigned)(T * nb)), dim3(256), 0, ctx->stream, base,
                       col_stride, A, lda, cols, p, ycol, beta, rank, bits, resid);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

static bool risk_ewma_ok(double half_life, int min_obs, int lag) {
    return std::isfinite(half_life) && half_life > 0.0 && min_obs >= 1 && lag >= 0;
}

extern "C" int afm_risk_factor_cov_f64(afm_ctx* ctx, const double* beta, const int32_t* rank,
                                       int64_t T, int p, double half_life, int min_obs, int lag,
                                       double* fcov, int32_t* nused) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(p >= 1 && p < kMaxF, "need 1 <= p and p + 1 <= AFM_RISK_MAX_FACTORS");
    AFM_CHECK_ARG(T >= 1, "T < 1");
    AFM_CHECK_ARG(risk_ewma_ok(half_life, min_obs, lag),
                  "need half_life > 0 (finite), min_obs >= 1, lag >= 0");
    AFM_CHECK_ARG(beta && rank && fcov && nused, "null buffer");
    const double lam = std::pow(0.5, 1.0 / half_life);
    hipLaunchKernelGGL(risk_fcov_kernel, dim3(1), dim3(256), 0, ctx->stream, beta, rank, T, p, lam,
                       min_obs, lag, fcov, nused);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_risk_specific_f64(afm_ctx* ctx, const double* resid, int64_t T, int64_t A,
                                     int64_t lda, double half_life, int min_obs, int lag,
                                     double* spec, double* fill) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(risk_shape_ok(T, A, lda), "bad panel shape");
    AFM_CHECK_ARG(risk_ewma_ok(half_life, min_obs, lag),
                  "need half_life > 0 (finite), min_obs >= 1, lag >= 0");
    AFM_CHECK_ARG(resid && spec && fill, "null buffer");
    AFM_CHECK_ARG(T < ((int64_t)1 << 31) && lda / 64 < ((int64_t)1 << 31), "too large for one launch");
    const double lam = std::pow(0.5, 1.0 / half_life);
    hipLaunchKernelGGL(risk_spec_kernel, dim3((unsigned)(lda / 64)), dim3(64), 0, ctx->stream, resid,
                       T, A, lda, lam, min_obs, lag, spec);
    AFM_HIP(hipGetLastError());
    const size_t smem = sizeof(double) * (kRun + 256);
    AFM_HIP(afm_lds_opt_in(ctx, (const void*)risk_fill_kernel, (int)smem));
    hipLaunchKernelGGL(risk_fill_kernel, dim3((unsigned)T), dim3(256), smem, ctx->stream,
                       (const double*)spec, A, lda, fill);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_risk_book_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                                 int64_t lda, const int32_t* cols, int p, const int32_t* dates,
                                 int64_t nd, const int32_t* k, const int32_t* books,
                                 const double* weights, const double* fcov, const double* spec,
                                 const double* fill, int kc, double* cov, double* risk,
                                 double* contrib, int32_t* status) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(p >= 1 && p < kMaxF, "need 1 <= p and p + 1 <= AFM_RISK_MAX_FACTORS");
    AFM_CHECK_ARG(T >= 1 && lda >= 64 && lda % 64 == 0, "bad panel shape");
    AFM_CHECK_ARG(kc >= 1 && kc <= kBook, "kc must be in [max k, 128]");
    AFM_CHECK_ARG(base && cols && dates && k && books && weights && fcov && spec && fill && cov &&
                      risk && contrib && status, "null buffer");
    AFM_CHECK_ARG(nd >= 0 && nd < ((int64_t)1 << 31), "bad nd");
    if (nd == 0) return AFM_OK;
    AFM_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)nd, ctx->stream));
    BookArgs r{base, col_stride, T, lda, cols, p, dates, k, books, weights, fcov, spec, fill, kc,
               cov, risk, contrib, status};
    const size_t smem = sizeof(BookLds);
    AFM_HIP(afm_lds_opt_in(ctx, (const void*)risk_book_kernel, (int)smem));
    hipLaunchKernelGGL(risk_book_kernel, dim3((unsigned)nd, 3), dim3(256), smem, ctx->stream, r);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
