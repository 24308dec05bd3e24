// Ensembles of small dense networks (include/afm_mlp.h): M networks p -> h1 -> h2 -> 1 fitted
// side by side with Adam, one workgroup of 256 threads (4 waves) per network and no communication
// between workgroups.  Every layer product and every gradient product runs on
// v_mfma_f64_16x16x4_f64 (operand layout as in xcorr.hip: lane l gives A[l & 15][l >> 4] and
// B[l >> 4][l & 15], entry r of its result is D[(l >> 4) + 4 r][l & 15]).
//
//  mlp_fit_kernel      the model's parameters theta[P] sit in LDS for the whole launch.  A step:
//                        F. the batch streams through in tiles of 16 rows: layer 1 (A = 16
//                           consecutive rows of one column plane from global, B = W1 from LDS), a1
//                           to an LDS tile, layer 2, a2 to an LDS tile, the output layer and d on
//                           wave 0 (with the epoch's running moments), d2 in place of a2, d1 = (d2
//                           W2') . [a1 > 0].  a1, d1, a2, d2 and d of the batch go to the model's
//                           scratch (L2): the gradient products run over the rows of the whole
//                           batch.
//                        G. the 16 x 16 tiles of the gradients -- W1, b1, W2, b2, w3, b3, the bias
//                           and w3 tiles with a ones / broadcast operand -- are dealt to the four
//                           waves; a wave sums one tile over the batch's rows in row order and
//                           applies Adam to its entries (m and v in scratch).  The outputs are
//                           split over the waves, not the rows: no cross-wave sum, a fixed order.
//                      At an epoch's end: the train moments, the eval rows through the forward
//                      tiles, the snapshot.  A launch runs the steps [step0, step1) and leaves
//                      theta, m, v, b1p, b2p and the running moments in global memory.
//  mlp_forward_kernel  workgroup (model, group of 64-row tiles): theta to LDS, the forward tiles.
//
// Masked rows (a short batch, the end of a range) load 0.0 in place of X and y and give d = 0:
// nothing of a row outside the range reaches a sum.
#include "afm_internal.h"
#include "afm_mlp.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace afm {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMlpThreads = 256;
constexpr int kMlpRows = 16;                  // rows of a tile
constexpr int kMlpPad = 2;                    // LDS tile row padding (doubles)
constexpr int kMlpState = 16;                 // doubles of the step state in scratch
constexpr int64_t kMlpDefaultSteps = 256;     // steps per launch when the option is 0
constexpr int kMlpFwdGroups = 64;             // forward: workgroups per model at most

struct MlpShape {
    int p, p4, h1, h2;
    int ob1, oW2, ob2, ow3, ob3, P;           // offsets into theta
    int S1, S2;                               // LDS tile row strides
};

MlpShape mlp_shape(int p, int h1, int h2) {
    MlpShape s;
    s.p = p;
    s.p4 = (p + 3) / 4 * 4;
    s.h1 = h1;
    s.h2 = h2;
    s.ob1 = p * h1;
    s.oW2 = s.ob1 + h1;
    s.ob2 = s.oW2 + h1 * h2;
    s.ow3 = s.ob2 + h2;
    s.ob3 = s.ow3 + h2;
    s.P = s.ob3 + 1;
    s.S1 = h1 + kMlpPad;
    s.S2 = h2 + kMlpPad;
    return s;
}

// LDS: theta[P rounded up to 2] | a1 tile [16][S1] | a2 tile [16][S2] | d [16]
__host__ __device__ inline int mlp_lds_doubles(const MlpShape& s) {
    return (s.P + 1) / 2 * 2 + kMlpRows * (s.S1 + s.S2) + kMlpRows;
}

// scratch of one model (doubles): m[Pp] | v[Pp] | state[16] | a1 [b16][h1] | d1 [b16][h1] |
// a2 [b16][h2] | d2 [b16][h2] | d [b16]
__host__ __device__ inline int64_t mlp_model_scratch(const MlpShape& s, int batch) {
    const int64_t Pp = (s.P + 1) / 2 * 2, b16 = (batch + 15) / 16 * 16;
    return 2 * Pp + kMlpState + b16 * (2 * (s.h1 + s.h2) + 1);
}

struct MlpLds {
    double* th;
    double* a1;
    double* a2;
    double* ds;
};

__device__ __forceinline__ MlpLds mlp_lds(double* smem, const MlpShape& s) {
    MlpLds l;
    l.th = smem;
    l.a1 = smem + (s.P + 1) / 2 * 2;
    l.a2 = l.a1 + kMlpRows * s.S1;
    l.ds = l.a2 + kMlpRows * s.S2;
    return l;
}

// The forward pass of the 16 rows from row0 (the first nv of them are real) with the parameters
// in LDS: a1 and a2 to their LDS tiles (TRAIN: also to ga1 / ga2 [16][h]); returns f of the rows
// (l >> 4) + 4 r on wave 0 (every lane), garbage on the other waves.  Two barriers inside; the
// caller may start the next tile without another one.
template <bool TRAIN>
__device__ __forceinline__ d4 mlp_forward_tile(const MlpShape& s, const MlpLds& l, const double* X,
                                               int64_t n_pad, int64_t row0, int nv, double* ga1,
                                               double* ga2) {
    const int lane = threadIdx.x & 63, fi = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const d4 zero4 = d4{0.0, 0.0, 0.0, 0.0};
    const bool rowok = fi < nv;
    for (int jt = wave; jt < s.h1 / 16; jt += 4) {
        d4 acc = zero4;
        const int col = 16 * jt + fi;
        for (int k0 = 0; k0 < s.p4; k0 += 4) {
            const int k = k0 + kk;
            const bool kok = k < s.p;
            const double a = kok && rowok ? X[(int64_t)k * n_pad + row0 + fi] : 0.0;
            const double b = kok ? l.th[k * s.h1 + col] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        const double bias = l.th[s.ob1 + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = kk + 4 * r;
            const double z = acc[r] + bias;
            const double a1 = z > 0.0 ? z : 0.0;
            l.a1[row * s.S1 + col] = a1;
            if constexpr (TRAIN) ga1[row * s.h1 + col] = a1;
        }
    }
    __syncthreads();
    for (int jt = wave; jt < s.h2 / 16; jt += 4) {
        d4 acc = zero4;
        const int col = 16 * jt + fi;
        for (int k0 = 0; k0 < s.h1; k0 += 4) {
            const int k = k0 + kk;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(l.a1[fi * s.S1 + k],
                                                       l.th[s.oW2 + k * s.h2 + col], acc, 0, 0, 0);
        }
        const double bias = l.th[s.ob2 + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = kk + 4 * r;
            const double z = acc[r] + bias;
            const double a2 = z > 0.0 ? z : 0.0;
            l.a2[row * s.S2 + col] = a2;
            if constexpr (TRAIN) ga2[row * s.h2 + col] = a2;
        }
    }
    __syncthreads();
    d4 f = zero4;
    if (wave == 0) {
        for (int k0 = 0; k0 < s.h2; k0 += 4) {
            const int k = k0 + kk;
            f = __builtin_amdgcn_mfma_f64_16x16x4f64(l.a2[fi * s.S2 + k], l.th[s.ow3 + k], f, 0, 0,
                                                     0);
        }
        const double b3 = l.th[s.ob3];
#pragma unroll
        for (int r = 0; r < 4; ++r) f[r] = f[r] + b3;
    }
    return f;
}

// the sum of x over the four row groups of a wave's lanes (fixed order); every lane gets it
__device__ __forceinline__ double mlp_rows_sum(double x) {
    x = x + __shfl_xor(x, 16);
    x = x + __shfl_xor(x, 32);
    return x;
}

// the six moments of the rows (l >> 4) + 4 r < nv of a tile added to mom (wave 0, every lane the
// same values): the tile's sums in a fixed order, then one add per moment
__device__ __forceinline__ void mlp_moments(const d4 f, const d4 y, int nv, double* mom) {
    const int kk = (threadIdx.x & 63) >> 4;
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (kk + 4 * r < nv) {
            t[0] = t[0] + 1.0;
            t[1] = t[1] + f[r];
            t[2] = t[2] + y[r];
            t[3] = t[3] + f[r] * f[r];
            t[4] = t[4] + y[r] * y[r];
            t[5] = t[5] + f[r] * y[r];
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) mom[j] = mom[j] + mlp_rows_sum(t[j]);
}

__device__ __forceinline__ d4 mlp_load_y(const double* y, int64_t row0, int nv) {
    const int kk = (threadIdx.x & 63) >> 4;
    d4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = kk + 4 * r < nv ? y[row0 + kk + 4 * r] : 0.0;
    return v;
}

struct MlpFitArgs {
    MlpShape s;
    const double* X;
    const double* y;
    int64_t n_pad, n_train, n_eval;
    double* theta;            // [M][P]
    const double* lr;         // [M] (device copy, in scratch)
    double beta1, beta2, eps;
    int batch, epochs;
    int64_t steps_per_epoch, step0, step1;
    double* evals;            // [M][epochs][2][6]
    double* snaps;            // [M][epochs][P] or null
    double* scratch;          // [M][model_scratch]
    int64_t model_scratch;
};

__global__ __launch_bounds__(kMlpThreads) void mlp_fit_kernel(MlpFitArgs g) {
    extern __shared__ double mlp_smem[];
    const MlpShape s = g.s;
    const MlpLds l = mlp_lds(mlp_smem, s);
    const int tid = threadIdx.x, lane = tid & 63, fi = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t model = blockIdx.x;
    const int P = s.P, h1 = s.h1, h2 = s.h2;
    const int64_t Pp = (P + 1) / 2 * 2, b16 = (g.batch + 15) / 16 * 16;
    double* theta = g.theta + model * P;
    double* sm = g.scratch + model * g.model_scratch;
    double* sv = sm + Pp;
    double* state = sv + Pp;
    double* ga1 = state + kMlpState;
    double* gd1 = ga1 + b16 * h1;
    double* ga2 = gd1 + b16 * h1;
    double* gd2 = ga2 + b16 * h2;
    double* gd = gd2 + b16 * h2;
    const d4 zero4 = d4{0.0, 0.0, 0.0, 0.0};

    for (int q = tid; q < P; q += kMlpThreads) l.th[q] = theta[q];
    double b1p = 1.0, b2p = 1.0, mom[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (g.step0 == 0) {
        for (int q = tid; q < P; q += kMlpThreads) {
            sm[q] = 0.0;
            sv[q] = 0.0;
        }
    } else {
        b1p = state[0];
        b2p = state[1];
#pragma unroll
        for (int j = 0; j < 6; ++j) mom[j] = state[2 + j];
    }
    const double lr = g.lr[model], c1 = 1.0 - g.beta1, c2 = 1.0 - g.beta2;
    __syncthreads();

    // the gradient tiles, in this order: W1 (ceil(p / 16) x h1 / 16), b1, W2, b2, w3, b3
    const int h1t = h1 / 16, h2t = h2 / 16, pt = (s.p + 15) / 16;
    const int e1 = pt * h1t, e2 = e1 + h1t, e3 = e2 + h1t * h2t, e4 = e3 + h2t, e5 = e4 + h2t;
    const int ntiles = e5 + 1;

    for (int64_t step = g.step0; step < g.step1; ++step) {
        const int64_t epoch = step / g.steps_per_epoch;
        const int64_t i0 = (step % g.steps_per_epoch) * g.batch;
        const int nb = (int)(g.n_train - i0 < g.batch ? g.n_train - i0 : g.batch);
        const double scale = 2.0 / (double)nb;
        const int nb16 = (nb + 15) / 16 * 16;

        // ---- F: forward and the deltas, tile by tile ------------------------------------------
        for (int r0 = 0; r0 < nb; r0 += kMlpRows) {
            const int nv = nb - r0 < kMlpRows ? nb - r0 : kMlpRows;
            const int64_t row0 = i0 + r0;
            const d4 f = mlp_forward_tile<true>(s, l, g.X, g.n_pad, row0, nv, ga1 + (int64_t)r0 * h1,
                                                ga2 + (int64_t)r0 * h2);
            if (wave == 0) {
                const d4 y = mlp_load_y(g.y, row0, nv);
                mlp_moments(f, y, nv, mom);
                if (fi == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = kk + 4 * r;
                        const double d = row < nv ? (f[r] - y[r]) * scale : 0.0;
                        l.ds[row] = d;
                        gd[r0 + row] = d;
                    }
                }
            }
            __syncthreads();
            for (int jt = wave; jt < h2t; jt += 4) {           // d2 in place of a2
                const int col = 16 * jt + fi;
                const double w3 = l.th[s.ow3 + col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = kk + 4 * r;
                    const double a2 = l.a2[row * s.S2 + col];
                    const double d2 = a2 > 0.0 ? l.ds[row] * w3 : 0.0;
                    l.a2[row * s.S2 + col] = d2;
                    gd2[(int64_t)(r0 + row) * h2 + col] = d2;
                }
            }
            __syncthreads();
            for (int jt = wave; jt < h1t; jt += 4) {           // d1 = (d2 W2') . [a1 > 0]
                d4 acc = zero4;
                const int col = 16 * jt + fi;
                for (int k0 = 0; k0 < h2; k0 += 4) {
                    const int k = k0 + kk;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(
                        l.a2[fi * s.S2 + k], l.th[s.oW2 + col * h2 + k], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = kk + 4 * r;
                    gd1[(int64_t)(r0 + row) * h1 + col] =
                        l.a1[row * s.S1 + col] > 0.0 ? acc[r] : 0.0;
                }
            }
            __syncthreads();
        }

        // ---- G: the gradient tiles over the batch's rows, then Adam -----------------------------
        b1p = b1p * g.beta1;
        b2p = b2p * g.beta2;
        const double lr_t = (lr * __builtin_sqrt(1.0 - b2p)) / (1.0 - b1p);
        for (int tt = wave; tt < ntiles; tt += 4) {
            d4 acc = zero4;
            int kind, ci = 0, cj = 0;
            if (tt < e1) { kind = 0; ci = tt / h1t; cj = tt % h1t; }
            else if (tt < e2) { kind = 1; cj = tt - e1; }
            else if (tt < e3) { kind = 2; ci = (tt - e2) / h2t; cj = (tt - e2) % h2t; }
            else if (tt < e4) { kind = 3; cj = tt - e3; }
            else if (tt < e5) { kind = 4; ci = tt - e4; }
            else { kind = 5; }
            if (kind == 0) {
                const int c = 16 * ci + fi;
                const bool cok = c < s.p;
                const double* xp = g.X + (int64_t)(cok ? c : 0) * g.n_pad + i0;
                const double* bp = gd1 + 16 * cj + fi;
                for (int r = 0; r < nb16; r += 4) {
                    const int row = r + kk;
                    const double a = cok && row < nb ? xp[row] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bp[(int64_t)row * h1], acc, 0, 0,
                                                               0);
                }
            } else if (kind == 1 || kind == 3) {
                const int hh = kind == 1 ? h1 : h2;
                const double* bp = (kind == 1 ? gd1 : gd2) + 16 * cj + fi;
                for (int r = 0; r < nb16; r += 4)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, bp[(int64_t)(r + kk) * hh], acc,
                                                               0, 0, 0);
            } else if (kind == 2) {
                const double* ap = ga1 + 16 * ci + fi;
                const double* bp = gd2 + 16 * cj + fi;
                for (int r = 0; r < nb16; r += 4) {
                    const int64_t row = r + kk;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[row * h1], bp[row * h2], acc, 0,
                                                               0, 0);
                }
            } else if (kind == 4) {
                const double* ap = ga2 + 16 * ci + fi;
                for (int r = 0; r < nb16; r += 4) {
                    const int64_t row = r + kk;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[row * h2], gd[row], acc, 0, 0, 0);
                }
            } else {
                for (int r = 0; r < nb16; r += 4)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, gd[r + kk], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = kk + 4 * r;                      // the entry's row of the tile
                int q = -1;
                if (kind == 0) { if (16 * ci + i < s.p) q = (16 * ci + i) * h1 + 16 * cj + fi; }
                else if (kind == 1) { if (i == 0) q = s.ob1 + 16 * cj + fi; }
                else if (kind == 2) { q = s.oW2 + (16 * ci + i) * h2 + 16 * cj + fi; }
                else if (kind == 3) { if (i == 0) q = s.ob2 + 16 * cj + fi; }
                else if (kind == 4) { if (fi == 0) q = s.ow3 + 16 * ci + i; }
                else { if (i == 0 && fi == 0) q = s.ob3; }
                if (q >= 0) {
                    const double gr = acc[r];
                    double m = sm[q], v = sv[q];
                    m = m + (gr - m) * c1;
                    v = v + (gr * gr - v) * c2;
                    sm[q] = m;
                    sv[q] = v;
                    l.th[q] = l.th[q] - (lr_t * m) / (__builtin_sqrt(v) + g.eps);
                }
            }
        }
        __syncthreads();

        // ---- the end of an epoch ---------------------------------------------------------------
        if ((step + 1) % g.steps_per_epoch == 0) {
            double* ev = g.evals + (model * g.epochs + epoch) * 12;
            if (tid == 0) {
#pragma unroll
                for (int j = 0; j < 6; ++j) ev[j] = mom[j];
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) mom[j] = 0.0;
            double em[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int64_t r0 = 0; r0 < g.n_eval; r0 += kMlpRows) {
                const int nv = (int)(g.n_eval - r0 < kMlpRows ? g.n_eval - r0 : kMlpRows);
                const int64_t row0 = g.n_train + r0;
                const d4 f = mlp_forward_tile<false>(s, l, g.X, g.n_pad, row0, nv, nullptr, nullptr);
                if (wave == 0) mlp_moments(f, mlp_load_y(g.y, row0, nv), nv, em);
            }
            if (tid == 0) {
#pragma unroll
                for (int j = 0; j < 6; ++j) ev[6 + j] = em[j];
            }
            if (g.snaps) {
                double* sn = g.snaps + (model * g.epochs + epoch) * P;
                for (int q = tid; q < P; q += kMlpThreads) sn[q] = l.th[q];
            }
            __syncthreads();
        }
    }

    for (int q = tid; q < P; q += kMlpThreads) theta[q] = l.th[q];
    if (tid == 0) {
        state[0] = b1p;
        state[1] = b2p;
#pragma unroll
        for (int j = 0; j < 6; ++j) state[2 + j] = mom[j];
    }
}

struct MlpFwdArgs {
    MlpShape s;
    const double* X;
    int64_t n_pad, i0, n;
    const double* theta;      // [M][P]
    double* out;              // [M][n_pad]
};

__global__ __launch_bounds__(kMlpThreads) void mlp_forward_kernel(MlpFwdArgs g) {
    extern __shared__ double mlp_smem[];
    const MlpShape s = g.s;
    const MlpLds l = mlp_lds(mlp_smem, s);
    const int tid = threadIdx.x, lane = tid & 63, fi = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t model = blockIdx.x;
    const double* theta = g.theta + model * s.P;
    double* out = g.out + model * g.n_pad;
    for (int q = tid; q < s.P; q += kMlpThreads) l.th[q] = theta[q];
    __syncthreads();
    const int64_t ntiles = (g.n + 63) / 64;
    for (int64_t t = blockIdx.y; t < ntiles; t += gridDim.y) {
        for (int sub = 0; sub < 4; ++sub) {
            const int64_t r0 = 64 * t + 16 * sub;
            if (r0 >= g.n) break;
            const int nv = (int)(g.n - r0 < kMlpRows ? g.n - r0 : kMlpRows);
            const int64_t row0 = g.i0 + r0;
            const d4 f = mlp_forward_tile<false>(s, l, g.X, g.n_pad, row0, nv, nullptr, nullptr);
            if (wave == 0 && fi == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kk + 4 * r < nv) out[row0 + kk + 4 * r] = f[r];
            }
        }
    }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// the shape rules of the header; empty when they hold
std::string mlp_shape_error(int p, int h1, int h2) {
    if (p < 1 || p > AFM_MLP_MAX_COLS) return "p must be in 1..64";
    if (h1 < 16 || h1 > AFM_MLP_MAX_HIDDEN || h1 % 16 || h2 < 16 || h2 > AFM_MLP_MAX_HIDDEN ||
        h2 % 16)
        return "h1 and h2 must be multiples of 16 in 16..128";
    if (h1 + h2 > AFM_MLP_MAX_WIDTH_SUM) return "h1 + h2 must be at most 192";
    if (h1 * ((p + 3) / 4 * 4 + h2) > AFM_MLP_MAX_WEIGHTS)
        return "h1 * (p4 + h2) must be at most 16384 (p4 = p rounded up to 4)";
    return "";
}

}  // namespace
}  // namespace afm

using namespace afm;

#define AFM_MLP_CHECK_VALUE(cond, msg)                             \
    do {                                                           \
        if (!(cond)) {                                             \
            afm_set_error(std::string(__func__) + ": " + (msg));   \
            return -1;                                             \
        }                                                          \
    } while (0)

extern "C" int64_t afm_mlp_param_count(int p, int h1, int h2) {
    const std::string e = mlp_shape_error(p, h1, h2);
    AFM_MLP_CHECK_VALUE(e.empty(), e);
    return mlp_shape(p, h1, h2).P;
}

extern "C" int64_t afm_mlp_scratch_bytes(int p, int h1, int h2, int M, int batch) {
    const std::string e = mlp_shape_error(p, h1, h2);
    AFM_MLP_CHECK_VALUE(e.empty(), e);
    AFM_MLP_CHECK_VALUE(M >= 1 && M <= AFM_MLP_MAX_MODELS, "M must be in 1..1024");
    AFM_MLP_CHECK_VALUE(batch >= 1 && batch <= AFM_MLP_MAX_BATCH, "batch must be in 1..4096");
    // the models' blocks, then the device copy of lr[M]
    const int64_t doubles = (int64_t)M * mlp_model_scratch(mlp_shape(p, h1, h2), batch) +
                            ((int64_t)M + 1) / 2 * 2;
    return (doubles * 8 + 255) / 256 * 256;
}

extern "C" int afm_mlp_fit_f64(afm_ctx* ctx, const double* X, const double* y, int64_t n_pad,
                               int64_t n_train, int64_t n_eval, int p, int h1, int h2, int M,
                               double* theta, const double* lr, double beta1, double beta2,
                               double eps, int batch, int epochs, double* evals, double* snaps,
                               double* scratch) {
    AFM_CTX(ctx);
    const std::string e = mlp_shape_error(p, h1, h2);
    AFM_CHECK_ARG(e.empty(), e);
    AFM_CHECK_ARG(M >= 1 && M <= AFM_MLP_MAX_MODELS, "M must be in 1..1024");
    AFM_CHECK_ARG(batch >= 1 && batch <= AFM_MLP_MAX_BATCH, "batch must be in 1..4096");
    AFM_CHECK_ARG(epochs >= 1 && epochs <= AFM_MLP_MAX_EPOCHS, "epochs must be in 1..4096");
    AFM_CHECK_ARG(n_pad >= 64 && n_pad % 64 == 0 && n_pad < (1ll << 31),
                  "n_pad: a multiple of 64 in 64..2^31");
    AFM_CHECK_ARG(n_train >= 1 && n_eval >= 0 && n_train <= n_pad && n_eval <= n_pad - n_train,
                  "need n_train >= 1, n_eval >= 0 and n_train + n_eval <= n_pad");
    AFM_CHECK_ARG(X && y && theta && lr && evals && scratch, "null buffer");
    AFM_CHECK_ARG(aligned16(X) && aligned16(y) && aligned16(theta) && aligned16(evals) &&
                      aligned16(snaps) && aligned16(scratch),
                  "X, y, theta, evals, snaps and scratch must be 16-byte aligned");
    AFM_CHECK_ARG(std::isfinite(eps) && eps > 0.0, "eps must be finite and > 0");
    AFM_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
                  "beta1 and beta2 must be in [0, 1)");
    for (int m = 0; m < M; ++m)
        AFM_CHECK_ARG(std::isfinite(lr[m]) && lr[m] > 0.0, "every lr must be finite and > 0");

    const MlpShape s = mlp_shape(p, h1, h2);
    const int lds = mlp_lds_doubles(s) * 8;
    AFM_HIP(afm_lds_opt_in(ctx, reinterpret_cast<const void*>(mlp_fit_kernel), lds));
    MlpFitArgs g;
    g.s = s;
    g.X = X;
    g.y = y;
    g.n_pad = n_pad;
    g.n_train = n_train;
    g.n_eval = n_eval;
    g.theta = theta;
    g.model_scratch = mlp_model_scratch(s, batch);
    double* dlr = scratch + (int64_t)M * g.model_scratch;
    g.lr = dlr;
    g.beta1 = beta1;
    g.beta2 = beta2;
    g.eps = eps;
    g.batch = batch;
    g.epochs = epochs;
    g.steps_per_epoch = (n_train + batch - 1) / batch;
    g.evals = evals;
    g.snaps = snaps;
    g.scratch = scratch;
    // lr is a host array the caller may free after the call: pageable memory is staged by the
    // runtime before hipMemcpyAsync returns
    AFM_HIP(hipMemcpyAsync(dlr, lr, sizeof(double) * M, hipMemcpyHostToDevice, ctx->stream));
    const int64_t total = g.steps_per_epoch * epochs;
    const int64_t S = ctx->mlp_steps_per_launch > 0 ? ctx->mlp_steps_per_launch : kMlpDefaultSteps;
    for (int64_t s0 = 0; s0 < total; s0 += S) {
        g.step0 = s0;
        g.step1 = std::min(total, s0 + S);
        hipLaunchKernelGGL(mlp_fit_kernel, dim3((unsigned)M), dim3(kMlpThreads), (size_t)lds,
                           ctx->stream, g);
    }
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_mlp_forward_f64(afm_ctx* ctx, const double* X, int64_t n_pad, int64_t i0,
                                   int64_t n, int p, int h1, int h2, int M, const double* theta,
                                   double* out) {
    AFM_CTX(ctx);
    const std::string e = mlp_shape_error(p, h1, h2);
    AFM_CHECK_ARG(e.empty(), e);
    AFM_CHECK_ARG(M >= 1 && M <= AFM_MLP_MAX_MODELS, "M must be in 1..1024");
    AFM_CHECK_ARG(n_pad >= 64 && n_pad % 64 == 0 && n_pad < (1ll << 31),
                  "n_pad: a multiple of 64 in 64..2^31");
    AFM_CHECK_ARG(i0 >= 0 && n >= 0 && i0 <= n_pad && n <= n_pad - i0,
                  "need i0 >= 0, n >= 0 and i0 + n <= n_pad");
    AFM_CHECK_ARG(X && theta && out, "null buffer");
    AFM_CHECK_ARG(aligned16(X) && aligned16(theta) && aligned16(out),
                  "X, theta and out must be 16-byte aligned");
    if (n == 0) return AFM_OK;
    const MlpShape s = mlp_shape(p, h1, h2);
    const int lds = mlp_lds_doubles(s) * 8;
    AFM_HIP(afm_lds_opt_in(ctx, reinterpret_cast<const void*>(mlp_forward_kernel), lds));
    MlpFwdArgs g{s, X, n_pad, i0, n, theta, out};
    const int64_t ntiles = (n + 63) / 64;
    const dim3 grid((unsigned)M, (unsigned)std::min<int64_t>(ntiles, kMlpFwdGroups));
    hipLaunchKernelGGL(mlp_forward_kernel, grid, dim3(kMlpThreads), (size_t)lds, ctx->stream, g);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
