// Ensembles of stacked LSTMs (include/afm_lstm.h): M networks LSTM(H1) -> LSTM(H2) -> Dense(1)
// fitted side by side with Adam.  A model's parameters (0.97 MB at the reference's widths) do not
// fit a workgroup's LDS, so they stay in global memory (L2) and a step is three kernels; the rows
// of a batch are independent through time, so no kernel synchronises across workgroups.  Every
// matrix product runs on v_mfma_f64_16x16x4_f64 (operand layout as in mlp.hip: lane l gives
// A[l & 15][l >> 4] and B[l >> 4][l & 15], entry r of its result is D[(l >> 4) + 4 r][l & 15]).
//
//  lstm_forward_kernel   workgroup (model, group of rows_per_wg batch rows), 4 waves.  It takes its
//                        rows 16 at a time and walks t = 0..T-1 through both layers: the h tiles
//                        (two buffers per layer) and the c tiles sit in LDS, K streams from L2 as
//                        the B operand.  The 16-wide tiles of hidden units are dealt to the waves;
//                        a wave holds the four gate sums of its (row, unit) entries in four
//                        accumulators, so the gates, c_t and h_t are formed in registers.  TRAIN:
//                        the gates, c_t, tanh(c_t) and h_t of every (t, row) go to the model's
//                        scratch, F and dF of the rows and the tile's six moments too.
//  lstm_backward_kernel  the same grid, t = T-1..0, layer 2 then layer 1 at every t: dz from the
//                        stored gates (written over them), then [dx | dh_next] = dz K' with K' as
//                        the B operand; dh_next, dc_next and layer 2's dx tile sit in LDS.
//  lstm_grad_kernel      the 16 x 16 tiles of dK1, db1, dK2, db2, dw, db3 (the bias and w tiles
//                        with a ones / broadcast operand) are dealt one to a wave; a wave sums its
//                        tile over (t, row) in that order and applies Adam to its entries (or
//                        writes the gradient out: afm_lstm_grad_f64).  Outputs are split, never
//                        summands: no cross-wave sum, one fixed order.
//  lstm_fold_kernel      adds the tiles' moments to the model's running moments in tile order.
//  lstm_epoch_kernel     the epoch's moments to evals, the snapshot.
//
// Masked rows (the end of a 16-row tile) load 0.0 in place of X and y and get dF = 0, so their dz
// is 0 at every step: nothing of a row outside the range reaches a sum.
#include "afm_internal.h"
#include "afm_lstm.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace afm {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kLstmThreads = 256;
constexpr int kLstmRows = 16;                 // rows of a tile
constexpr int kLstmPad = 2;                   // LDS tile row padding (doubles)
constexpr int kLstmState = 16;                // doubles of a model's running moments: train | eval
constexpr int kLstmParts = 64;                // tiles of one forward launch that writes moments
constexpr int kLstmDefaultRows = 16;          // rows of a workgroup when the option is 0
constexpr int kLstmMaxGroups = 256;           // workgroups per model at most (grid-stride beyond)

__device__ __forceinline__ double lstm_sig(double z) { return 1.0 / (1.0 + exp(-z)); }
__device__ __forceinline__ double lstm_tanh(double z) { return tanh(z); }

struct LstmShape {
    int T, d, h1, h2;
    int ob1, oK2, ob2, ow, ob3, P;            // offsets into theta (K1 at 0)
};

LstmShape lstm_shape(int T, int d, int h1, int h2) {
    LstmShape s;
    s.T = T;
    s.d = d;
    s.h1 = h1;
    s.h2 = h2;
    s.ob1 = (d + h1) * 4 * h1;
    s.oK2 = s.ob1 + 4 * h1;
    s.ob2 = s.oK2 + (h1 + h2) * 4 * h2;
    s.ow = s.ob2 + 4 * h2;
    s.ob3 = s.ow + h2;
    s.P = s.ob3 + 1;
    return s;
}

// scratch of one model (doubles) for batches of rows16 rows (a multiple of 16):
// m[Pp] | v[Pp] | state[16] | part[64][6] | dF[rows16] | per layer: gates / dz [T][rows16][4H],
// c, tanh(c), h [T][rows16][H]
struct LstmLayout {
    int64_t ov, ostate, opart, odF, oG1, oC1, oTC1, oH1, oG2, oC2, oTC2, oH2, total;
};

LstmLayout lstm_layout(const LstmShape& s, int rows16) {
    LstmLayout l;
    const int64_t Pp = (s.P + 1) / 2 * 2, n = (int64_t)s.T * rows16;
    l.ov = Pp;
    l.ostate = 2 * Pp;
    l.opart = l.ostate + kLstmState;
    l.odF = l.opart + kLstmParts * 6;
    l.oG1 = l.odF + rows16;
    l.oC1 = l.oG1 + n * 4 * s.h1;
    l.oTC1 = l.oC1 + n * s.h1;
    l.oH1 = l.oTC1 + n * s.h1;
    l.oG2 = l.oH1 + n * s.h1;
    l.oC2 = l.oG2 + n * 4 * s.h2;
    l.oTC2 = l.oC2 + n * s.h2;
    l.oH2 = l.oTC2 + n * s.h2;
    l.total = l.oH2 + n * s.h2;
    return l;
}

struct LstmArgs {
    LstmShape s;
    LstmLayout l;
    const double* X;
    const double* y;
    int64_t n_pad, i0, n;     // the rows [i0, i0 + n) of this launch
    int rows16;               // scratch row stride: n rounded up to 16 (train launches)
    int rows_per_wg;
    const double* theta;      // [M][P]
    double* scratch;          // [M][model_scratch], after the lr block
    int64_t model_scratch;
    double* out;              // [M][n_pad] or null
    double scale;             // 2.0 / nb
};

enum { kPredict = 0, kTrain = 1, kEval = 2 };

// One layer step of the 16 rows of a tile: z = [x | hprev] K + b on the MFMA, then the gates, c and
// h of the wave's (row, unit) entries.  L1: x from the planes xg (rows fi < nv, else 0.0); else
// from the LDS tile xl.  TRAIN: G, C, TC, Hs point at the tile's rows of the scratch slot t.
template <bool TRAIN, bool L1>
__device__ __forceinline__ void lstm_cell(const double* __restrict__ K,
                                          const double* __restrict__ bias, int din, int H,
                                          const double* __restrict__ xg, int64_t n_pad, int nv,
                                          const double* xl, int Sx, const double* hprev,
                                          double* hnew, double* c, int S, double* G, double* C,
                                          double* TC, double* Hs) {
    const int lane = threadIdx.x & 63, fi = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KK = (din + H + 3) / 4 * 4, H4 = 4 * H;
    const d4 zero4 = d4{0.0, 0.0, 0.0, 0.0};
    for (int ju = wave; ju < (H + 15) / 16; ju += 4) {
        const int col = 16 * ju + fi;
        const bool cok = col < H;
        d4 ai = zero4, af = zero4, ag = zero4, ao = zero4;
        for (int k0 = 0; k0 < KK; k0 += 4) {
            const int k = k0 + kk;
            double a = 0.0;
            if (k < din) {
                if constexpr (L1) a = fi < nv ? xg[(int64_t)k * n_pad + fi] : 0.0;
                else a = xl[fi * Sx + k];
            } else if (k < din + H) {
                a = hprev[fi * S + (k - din)];
            }
            const bool kok = cok && k < din + H;
            const double* kp = K + (int64_t)(kok ? k : 0) * H4 + (kok ? col : 0);
            const double bi = kok ? kp[0] : 0.0;
            const double bf = kok ? kp[H] : 0.0;
            const double bg = kok ? kp[2 * H] : 0.0;
            const double bo = kok ? kp[3 * H] : 0.0;
            ai = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bi, ai, 0, 0, 0);
            af = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bf, af, 0, 0, 0);
            ag = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bg, ag, 0, 0, 0);
            ao = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bo, ao, 0, 0, 0);
        }
        if (cok) {
            const double b_i = bias[col], b_f = bias[H + col], b_g = bias[2 * H + col],
                         b_o = bias[3 * H + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kk + 4 * r;
                const double gi = lstm_sig(ai[r] + b_i);
                const double gf = lstm_sig(af[r] + b_f);
                const double gg = lstm_tanh(ag[r] + b_g);
                const double go = lstm_sig(ao[r] + b_o);
                const double cn = gf * c[row * H + col] + gi * gg;
                const double tc = lstm_tanh(cn);
                const double h = go * tc;
                c[row * H + col] = cn;
                hnew[row * S + col] = h;
                if constexpr (TRAIN) {
                    double* gp = G + (int64_t)row * H4 + col;
                    gp[0] = gi;
                    gp[H] = gf;
                    gp[2 * H] = gg;
                    gp[3 * H] = go;
                    C[(int64_t)row * H + col] = cn;
                    TC[(int64_t)row * H + col] = tc;
                    Hs[(int64_t)row * H + col] = h;
                }
            }
        }
    }
}

// LDS of the forward kernel: h1[2][16][S1] | h2[2][16][S2] | c1[16][h1] | c2[16][h2] | f[16]
__host__ __device__ inline int lstm_fwd_lds_doubles(int h1, int h2) {
    return kLstmRows * (2 * (h1 + kLstmPad) + 2 * (h2 + kLstmPad) + h1 + h2) + kLstmRows;
}

template <int MODE>
__global__ __launch_bounds__(kLstmThreads) void lstm_forward_kernel(LstmArgs g) {
    extern __shared__ double lstm_smem[];
    constexpr bool TRAIN = MODE == kTrain;
    const LstmShape s = g.s;
    const int tid = threadIdx.x, lane = tid & 63, fi = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t model = blockIdx.x;
    const int T = s.T, d = s.d, h1 = s.h1, h2 = s.h2, S1 = h1 + kLstmPad, S2 = h2 + kLstmPad;
    const double* theta = g.theta + model * s.P;
    double* sc = g.scratch ? g.scratch + model * g.model_scratch : nullptr;
    double* hb1 = lstm_smem;
    double* hb2 = hb1 + 2 * kLstmRows * S1;
    double* c1 = hb2 + 2 * kLstmRows * S2;
    double* c2 = c1 + kLstmRows * h1;
    double* fs = c2 + kLstmRows * h2;
    const int R = g.rows_per_wg;
    const int64_t ngroups = (g.n + R - 1) / R;
    const d4 zero4 = d4{0.0, 0.0, 0.0, 0.0};

    for (int64_t grp = blockIdx.y; grp < ngroups; grp += gridDim.y) {
        for (int sub = 0; sub < R; sub += kLstmRows) {
            const int64_t r0 = grp * R + sub;             // the tile's first row within the launch
            if (r0 >= g.n) break;
            const int nv = (int)(g.n - r0 < kLstmRows ? g.n - r0 : kLstmRows);
            const int64_t row0 = g.i0 + r0;
            for (int q = tid; q < kLstmRows * S1; q += kLstmThreads) hb1[q] = 0.0;
            for (int q = tid; q < kLstmRows * S2; q += kLstmThreads) hb2[q] = 0.0;
            for (int q = tid; q < kLstmRows * (h1 + h2); q += kLstmThreads) c1[q] = 0.0;
            __syncthreads();
            for (int t = 0; t < T; ++t) {
                const int cur = t & 1, nxt = cur ^ 1;
                double *G1 = nullptr, *C1 = nullptr, *TC1 = nullptr, *H1 = nullptr;
                double *G2 = nullptr, *C2 = nullptr, *TC2 = nullptr, *H2 = nullptr;
                if constexpr (TRAIN) {
                    const int64_t slot = (int64_t)t * g.rows16 + r0;
                    G1 = sc + g.l.oG1 + slot * 4 * h1;
                    C1 = sc + g.l.oC1 + slot * h1;
                    TC1 = sc + g.l.oTC1 + slot * h1;
                    H1 = sc + g.l.oH1 + slot * h1;
                    G2 = sc + g.l.oG2 + slot * 4 * h2;
                    C2 = sc + g.l.oC2 + slot * h2;
                    TC2 = sc + g.l.oTC2 + slot * h2;
                    H2 = sc + g.l.oH2 + slot * h2;
                }
                lstm_cell<TRAIN, true>(theta, theta + s.ob1, d, h1,
                                       g.X + (int64_t)t * d * g.n_pad + row0, g.n_pad, nv, nullptr,
                                       0, hb1 + cur * kLstmRows * S1, hb1 + nxt * kLstmRows * S1, c1,
                                       S1, G1, C1, TC1, H1);
                __syncthreads();
                lstm_cell<TRAIN, false>(theta + s.oK2, theta + s.ob2, h1, h2, nullptr, 0, nv,
                                        hb1 + nxt * kLstmRows * S1, S1, hb2 + cur * kLstmRows * S2,
                                        hb2 + nxt * kLstmRows * S2, c2, S2, G2, C2, TC2, H2);
                __syncthreads();
            }
            const double* hT = hb2 + (T & 1) * kLstmRows * S2;
            if (wave == 0) {
                d4 f = zero4;
                for (int k0 = 0; k0 < h2; k0 += 4)
                    f = __builtin_amdgcn_mfma_f64_16x16x4f64(hT[fi * S2 + k0 + kk],
                                                             theta[s.ow + k0 + kk], f, 0, 0, 0);
                const double b3 = theta[s.ob3];
                if (fi == 0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = kk + 4 * r;
                        const double F = f[r] + b3;
                        fs[row] = F;
                        if (row < nv && g.out) g.out[model * g.n_pad + row0 + row] = F;
                        if constexpr (TRAIN)
                            sc[g.l.odF + r0 + row] =
                                row < nv ? (F - g.y[row0 + row]) * g.scale : 0.0;
                    }
                }
            }
            __syncthreads();
            if constexpr (MODE != kPredict) {
                if (tid == 0) {                           // the tile's moments, row after row
                    double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    for (int row = 0; row < nv; ++row) {
                        const double F = fs[row], yy = g.y[row0 + row];
                        p[0] = p[0] + 1.0;
                        p[1] = p[1] + F;
                        p[2] = p[2] + yy;
                        p[3] = p[3] + F * F;
                        p[4] = p[4] + yy * yy;
                        p[5] = p[5] + F * yy;
                    }
                    double* part = sc + g.l.opart + (r0 / kLstmRows) * 6;
#pragma unroll
                    for (int j = 0; j < 6; ++j) part[j] = p[j];
                }
            }
            __syncthreads();
        }
    }
}

// dz of the tile's rows of one layer at step t from the stored gates (written over them in scratch
// and to the LDS tile dz [16][SZ]); dc_next in place.  dh = dh_in + dh_next with dh_in = dF (x) w
// (w non-null), din[row][j] (din non-null) or 0.0.
__device__ __forceinline__ void lstm_dz(int H, int t, double* G, const double* C, const double* TC,
                                        int64_t rows16, int64_t r0, const double* w,
                                        const double* dFs, const double* din, const double* dhn,
                                        double* dcn, double* dz, int SZ) {
    const int H4 = 4 * H;
    for (int e = threadIdx.x; e < kLstmRows * H; e += kLstmThreads) {
        const int row = e / H, j = e - row * H;
        const int64_t slot = (int64_t)t * rows16 + r0 + row;
        double* gp = G + slot * H4 + j;
        const double gi = gp[0], gf = gp[H], gg = gp[2 * H], go = gp[3 * H];
        const double tc = TC[slot * H + j];
        const double cp = t > 0 ? C[(slot - rows16) * H + j] : 0.0;
        const double dh_in = w ? dFs[row] * w[j] : (din ? din[row * H + j] : 0.0);
        const double dh = dh_in + dhn[row * H + j];
        const double d_o = dh * tc;
        const double dc = (dh * go) * (1.0 - tc * tc) + dcn[row * H + j];
        const double di = dc * gg, dg = dc * gi, df = dc * cp;
        dcn[row * H + j] = dc * gf;
        const double zi = (di * gi) * (1.0 - gi);
        const double zf = (df * gf) * (1.0 - gf);
        const double zg = dg * (1.0 - gg * gg);
        const double zo = (d_o * go) * (1.0 - go);
        gp[0] = zi;
        gp[H] = zf;
        gp[2 * H] = zg;
        gp[3 * H] = zo;
        double* zp = dz + row * SZ + j;
        zp[0] = zi;
        zp[H] = zf;
        zp[2 * H] = zg;
        zp[3 * H] = zo;
    }
}

// out[row][nn] = sum_k dz[row][k] K[n_lo + nn][k] for nn in [0, n_cnt): the 16-wide tiles of nn are
// dealt to the waves; nn < split goes to o1 [16][split], the rest to o2 [16][n_cnt - split]
__device__ __forceinline__ void lstm_back_prod(const double* __restrict__ K, int H4, int n_lo,
                                               int n_cnt, const double* dz, int SZ, int split,
                                               double* o1, double* o2) {
    const int lane = threadIdx.x & 63, fi = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int jt = wave; jt < (n_cnt + 15) / 16; jt += 4) {
        const int nn = 16 * jt + fi;
        const bool nok = nn < n_cnt;
        const double* kp = K + (int64_t)(nok ? n_lo + nn : 0) * H4 + kk;
        const double* ap = dz + fi * SZ + kk;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < H4; k0 += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[k0], nok ? kp[k0] : 0.0, acc, 0, 0, 0);
        if (nok) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kk + 4 * r;
                if (nn < split) o1[row * split + nn] = acc[r];
                else o2[row * (n_cnt - split) + (nn - split)] = acc[r];
            }
        }
    }
}

// LDS of the backward kernel: dz[16][4 max(h1, h2) + pad] | dh1n, dc1n, dx [16][h1] | dh2n, dc2n
// [16][h2] | dF[16]
__host__ __device__ inline int lstm_bwd_lds_doubles(int h1, int h2) {
    const int hm = h1 > h2 ? h1 : h2;
    return kLstmRows * (4 * hm + kLstmPad + 3 * h1 + 2 * h2) + kLstmRows;
}

__global__ __launch_bounds__(kLstmThreads) void lstm_backward_kernel(LstmArgs g) {
    extern __shared__ double lstm_smem[];
    const LstmShape s = g.s;
    const int tid = threadIdx.x;
    const int64_t model = blockIdx.x;
    const int T = s.T, d = s.d, h1 = s.h1, h2 = s.h2, hm = h1 > h2 ? h1 : h2;
    const int SZ = 4 * hm + kLstmPad;
    const double* theta = g.theta + model * s.P;
    double* sc = g.scratch + model * g.model_scratch;
    double* dz = lstm_smem;
    double* dh1n = dz + kLstmRows * SZ;
    double* dc1n = dh1n + kLstmRows * h1;
    double* dx = dc1n + kLstmRows * h1;
    double* dh2n = dx + kLstmRows * h1;
    double* dc2n = dh2n + kLstmRows * h2;
    double* dFs = dc2n + kLstmRows * h2;
    const int R = g.rows_per_wg;
    const int64_t ngroups = (g.n + R - 1) / R;

    for (int64_t grp = blockIdx.y; grp < ngroups; grp += gridDim.y) {
        for (int sub = 0; sub < R; sub += kLstmRows) {
            const int64_t r0 = grp * R + sub;
            if (r0 >= g.n) break;
            for (int q = tid; q < kLstmRows * (3 * h1 + 2 * h2); q += kLstmThreads) dh1n[q] = 0.0;
            if (tid < kLstmRows) dFs[tid] = sc[g.l.odF + r0 + tid];
            __syncthreads();
            for (int t = T - 1; t >= 0; --t) {
                lstm_dz(h2, t, sc + g.l.oG2, sc + g.l.oC2, sc + g.l.oTC2, g.rows16, r0,
                        t == T - 1 ? theta + s.ow : nullptr, dFs, nullptr, dh2n, dc2n, dz, SZ);
                __syncthreads();
                lstm_back_prod(theta + s.oK2, 4 * h2, 0, h1 + h2, dz, SZ, h1, dx, dh2n);
                __syncthreads();
                lstm_dz(h1, t, sc + g.l.oG1, sc + g.l.oC1, sc + g.l.oTC1, g.rows16, r0, nullptr,
                        dFs, dx, dh1n, dc1n, dz, SZ);
                __syncthreads();
                lstm_back_prod(theta, 4 * h1, d, h1, dz, SZ, h1, dh1n, nullptr);
                __syncthreads();
            }
        }
    }
}

struct LstmGradArgs {
    LstmShape s;
    LstmLayout l;
    const double* X;
    int64_t n_pad, i0;
    int nb, rows16;
    double* theta;            // [M][P]
    double* scratch;
    int64_t model_scratch;
    const double* lr;         // [M] (device copy, in scratch)
    double b1p, b2p, c1, c2, eps;
    double* gout;             // [M][P]: the gradient is written here and nothing is updated
};

__global__ __launch_bounds__(kLstmThreads) void lstm_grad_kernel(LstmGradArgs g) {
    const LstmShape s = g.s;
    const int lane = threadIdx.x & 63, fi = lane & 15, kk = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t model = blockIdx.y;
    const int T = s.T, d = s.d, h1 = s.h1, h2 = s.h2, nb = g.nb;
    const int64_t rows16 = g.rows16;
    double* theta = g.theta + model * s.P;
    double* sc = g.scratch + model * g.model_scratch;
    const double* dF = sc + g.l.odF;
    // the tiles, in this order: K1 (ceil((d + h1) / 16) x 4 h1 / 16), b1, K2, b2, w, b3
    const int g1 = 4 * h1 / 16, g2 = 4 * h2 / 16;
    const int r1 = (d + h1 + 15) / 16, r2 = (h1 + h2 + 15) / 16;
    const int e1 = r1 * g1, e2 = e1 + g1, e3 = e2 + r2 * g2, e4 = e3 + g2, e5 = e4 + (h2 + 15) / 16;
    const int tt = blockIdx.x * 4 + wave;
    if (tt > e5) return;
    int kind, ci = 0, cj = 0;
    if (tt < e1) { kind = 0; ci = tt / g1; cj = tt % g1; }
    else if (tt < e2) { kind = 1; cj = tt - e1; }
    else if (tt < e3) { kind = 2; ci = (tt - e2) / g2; cj = (tt - e2) % g2; }
    else if (tt < e4) { kind = 3; cj = tt - e3; }
    else if (tt < e5) { kind = 4; ci = tt - e4; }
    else { kind = 5; }

    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    if (kind <= 3) {
        const bool first = kind <= 1;
        const int H = first ? h1 : h2, H4 = 4 * H, din = first ? d : h1;
        const double* Z = sc + (first ? g.l.oG1 : g.l.oG2) + 16 * cj + fi;
        const double* Hown = sc + (first ? g.l.oH1 : g.l.oH2);
        const double* Hlow = sc + g.l.oH1;                    // layer 2's input
        const int c = 16 * ci + fi;                           // the row of K this lane feeds
        const bool bias = kind == 1 || kind == 3;
        for (int t = 0; t < T; ++t) {
            const int64_t base = (int64_t)t * rows16;
            for (int r = 0; r < rows16; r += 4) {
                const int row = r + kk;
                double a;
                if (bias) {
                    a = 1.0;
                } else if (c < din) {
                    if (first) a = row < nb ? g.X[((int64_t)t * d + c) * g.n_pad + g.i0 + row] : 0.0;
                    else a = Hlow[(base + row) * h1 + c];
                } else if (c < din + H && t > 0) {
                    a = Hown[(base - rows16 + row) * H + (c - din)];
                } else {
                    a = 0.0;
                }
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Z[(base + row) * H4], acc, 0, 0, 0);
            }
        }
    } else {
        const int c = 16 * ci + fi;
        const double* hT = sc + g.l.oH2 + (int64_t)(T - 1) * rows16 * h2;
        for (int r = 0; r < rows16; r += 4) {
            const int row = r + kk;
            const double a = kind == 5 ? 1.0 : (c < h2 ? hT[(int64_t)row * h2 + c] : 0.0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, dF[row], acc, 0, 0, 0);
        }
    }

    double* sm = sc;
    double* sv = sc + g.l.ov;
    const double lr_t = g.gout ? 0.0 : (g.lr[model] * __builtin_sqrt(1.0 - g.b2p)) / (1.0 - g.b1p);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = kk + 4 * r;                             // the entry's row of the tile
        int q = -1;
        if (kind == 0) { if (16 * ci + i < d + h1) q = (16 * ci + i) * 4 * h1 + 16 * cj + fi; }
        else if (kind == 1) { if (i == 0) q = s.ob1 + 16 * cj + fi; }
        else if (kind == 2) { if (16 * ci + i < h1 + h2) q = s.oK2 + (16 * ci + i) * 4 * h2 + 16 * cj + fi; }
        else if (kind == 3) { if (i == 0) q = s.ob2 + 16 * cj + fi; }
        else if (kind == 4) { if (fi == 0 && 16 * ci + i < h2) q = s.ow + 16 * ci + i; }
        else { if (i == 0 && fi == 0) q = s.ob3; }
        if (q >= 0) {
            const double gr = acc[r];
            if (g.gout) {
                g.gout[model * s.P + q] = gr;
            } else {
                double m = sm[q], v = sv[q];
                m = m + (gr - m) * g.c1;
                v = v + (gr * gr - v) * g.c2;
                sm[q] = m;
                sv[q] = v;
                theta[q] = theta[q] - (lr_t * m) / (__builtin_sqrt(v) + g.eps);
            }
        }
    }
}

// state[which * 8 + j] += part[k][j] for k = 0..ntiles-1, in that order
__global__ void lstm_fold_kernel(double* scratch, int64_t model_scratch, int64_t ostate,
                                 int64_t opart, int which, int ntiles) {
    double* sc = scratch + blockIdx.x * model_scratch;
    const int j = threadIdx.x;
    if (j >= 6) return;
    double a = sc[ostate + which * 8 + j];
    for (int k = 0; k < ntiles; ++k) a = a + sc[opart + k * 6 + j];
    sc[ostate + which * 8 + j] = a;
}

// zero m, v and the running moments of every model
__global__ void lstm_init_kernel(double* scratch, int64_t model_scratch, int64_t count) {
    double* sc = scratch + blockIdx.y * model_scratch;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < count;
         q += (int64_t)gridDim.x * blockDim.x)
        sc[q] = 0.0;
}

// the end of an epoch: the running moments to evals (and back to zero), the snapshot
__global__ void lstm_epoch_kernel(double* scratch, int64_t model_scratch, int64_t ostate,
                                  const double* theta, int P, double* evals, double* snaps,
                                  int epochs, int epoch) {
    const int64_t model = blockIdx.y;
    double* st = scratch + model * model_scratch + ostate;
    if (blockIdx.x == 0 && threadIdx.x < 12) {
        const int which = threadIdx.x / 6, j = threadIdx.x % 6;
        evals[((model * epochs + epoch) * 2 + which) * 6 + j] = st[which * 8 + j];
        st[which * 8 + j] = 0.0;
    }
    if (snaps) {
        double* sn = snaps + (model * epochs + epoch) * P;
        const double* th = theta + model * P;
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < P; q += gridDim.x * blockDim.x)
            sn[q] = th[q];
    }
}

__global__ void lstm_act_kernel(int kind, const double* x, int64_t n, double* out) {
    const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (q < n) out[q] = kind == 0 ? lstm_sig(x[q]) : lstm_tanh(x[q]);
}

bool lstm_aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// the shape rules of the header; empty when they hold
std::string lstm_shape_error(int T, int d, int h1, int h2) {
    if (T < 1 || T > AFM_LSTM_MAX_STEPS) return "T must be in 1..256";
    if (d < 1 || d > AFM_LSTM_MAX_INPUTS) return "d must be in 1..64";
    if (h1 < 4 || h1 > AFM_LSTM_MAX_HIDDEN || h1 % 4 || h2 < 4 || h2 > AFM_LSTM_MAX_HIDDEN || h2 % 4)
        return "h1 and h2 must be multiples of 4 in 4..128";
    return "";
}

int lstm_rows_per_wg(const afm_ctx* ctx) {
    return ctx->lstm_rows_per_wg > 0 ? ctx->lstm_rows_per_wg : kLstmDefaultRows;
}

dim3 lstm_grid(int M, int64_t n, int R) {
    return dim3((unsigned)M, (unsigned)std::min<int64_t>((n + R - 1) / R, kLstmMaxGroups));
}

template <int MODE>
hipError_t lstm_launch_forward(afm_ctx* ctx, const LstmArgs& g, int M) {
    const int lds = lstm_fwd_lds_doubles(g.s.h1, g.s.h2) * 8;
    const hipError_t e =
        afm_lds_opt_in(ctx, reinterpret_cast<const void*>(lstm_forward_kernel<MODE>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lstm_forward_kernel<MODE>, lstm_grid(M, g.n, g.rows_per_wg),
                       dim3(kLstmThreads), (size_t)lds, ctx->stream, g);
    return hipSuccess;
}

// forward (TRAIN), the fold of the batch's moments, backward and the gradient tiles of one batch
hipError_t lstm_launch_step(afm_ctx* ctx, LstmArgs g, LstmGradArgs q, int M, bool fold) {
    hipError_t e = lstm_launch_forward<kTrain>(ctx, g, M);
    if (e != hipSuccess) return e;
    if (fold)
        hipLaunchKernelGGL(lstm_fold_kernel, dim3((unsigned)M), dim3(64), 0, ctx->stream, g.scratch,
                           g.model_scratch, g.l.ostate, g.l.opart, 0, g.rows16 / kLstmRows);
    const int lds = lstm_bwd_lds_doubles(g.s.h1, g.s.h2) * 8;
    e = afm_lds_opt_in(ctx, reinterpret_cast<const void*>(lstm_backward_kernel), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lstm_backward_kernel, lstm_grid(M, g.n, g.rows_per_wg), dim3(kLstmThreads),
                       (size_t)lds, ctx->stream, g);
    const LstmShape& s = g.s;
    const int ntiles = ((s.d + s.h1 + 15) / 16 + 1) * (s.h1 / 4) +
                       ((s.h1 + s.h2 + 15) / 16 + 1) * (s.h2 / 4) + (s.h2 + 15) / 16 + 1;
    hipLaunchKernelGGL(lstm_grad_kernel, dim3((unsigned)((ntiles + 3) / 4), (unsigned)M),
                       dim3(kLstmThreads), 0, ctx->stream, q);
    return hipSuccess;
}

}  // namespace
}  // namespace afm

using namespace afm;

#define AFM_LSTM_CHECK_VALUE(cond, msg)                            \
    do {                                                           \
        if (!(cond)) {                                             \
            afm_set_error(std::string(__func__) + ": " + (msg));   \
            return -1;                                             \
        }                                                          \
    } while (0)

extern "C" int64_t afm_lstm_param_count(int d, int h1, int h2) {
    const std::string e = lstm_shape_error(1, d, h1, h2);
    AFM_LSTM_CHECK_VALUE(e.empty(), e);
    return lstm_shape(1, d, h1, h2).P;
}

extern "C" int64_t afm_lstm_scratch_bytes(int T, int d, int h1, int h2, int M, int batch) {
    const std::string e = lstm_shape_error(T, d, h1, h2);
    AFM_LSTM_CHECK_VALUE(e.empty(), e);
    AFM_LSTM_CHECK_VALUE(M >= 1 && M <= AFM_LSTM_MAX_MODELS, "M must be in 1..64");
    AFM_LSTM_CHECK_VALUE(batch >= 1 && batch <= AFM_LSTM_MAX_BATCH, "batch must be in 1..1024");
    // the device copy of lr[M], then the models' blocks
    const int64_t doubles = AFM_LSTM_MAX_MODELS +
        (int64_t)M * lstm_layout(lstm_shape(T, d, h1, h2), (batch + 15) / 16 * 16).total;
    return (doubles * 8 + 255) / 256 * 256;
}

#define AFM_LSTM_CHECK_COMMON(n_pad)                                                        \
    const std::string shape_err = lstm_shape_error(T, d, h1, h2);                           \
    AFM_CHECK_ARG(shape_err.empty(), shape_err);                                            \
    AFM_CHECK_ARG(M >= 1 && M <= AFM_LSTM_MAX_MODELS, "M must be in 1..64");                \
    AFM_CHECK_ARG(n_pad >= 64 && n_pad % 64 == 0 && n_pad < (1ll << 31),                    \
                  "n_pad: a multiple of 64 in 64..2^31")

extern "C" int afm_lstm_fit_f64(afm_ctx* ctx, const double* X, const double* y, int64_t n_pad,
                                int64_t n_train, int64_t n_eval, int T, int d, int h1, int h2,
                                int M, double* theta, const double* lr, double beta1, double beta2,
                                double eps, int batch, int epochs, double* evals, double* snaps,
                                double* scratch) {
    AFM_CTX(ctx);
    AFM_LSTM_CHECK_COMMON(n_pad);
    AFM_CHECK_ARG(batch >= 1 && batch <= AFM_LSTM_MAX_BATCH, "batch must be in 1..1024");
    AFM_CHECK_ARG(epochs >= 1 && epochs <= AFM_LSTM_MAX_EPOCHS, "epochs must be in 1..4096");
    AFM_CHECK_ARG(n_train >= 1 && n_eval >= 0 && n_train <= n_pad && n_eval <= n_pad - n_train,
                  "need n_train >= 1, n_eval >= 0 and n_train + n_eval <= n_pad");
    AFM_CHECK_ARG(X && y && theta && lr && evals && scratch, "null buffer");
    AFM_CHECK_ARG(lstm_aligned16(X) && lstm_aligned16(y) && lstm_aligned16(theta) &&
                      lstm_aligned16(evals) && lstm_aligned16(snaps) && lstm_aligned16(scratch),
                  "X, y, theta, evals, snaps and scratch must be 16-byte aligned");
    AFM_CHECK_ARG(std::isfinite(eps) && eps > 0.0, "eps must be finite and > 0");
    AFM_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
                  "beta1 and beta2 must be in [0, 1)");
    for (int m = 0; m < M; ++m)
        AFM_CHECK_ARG(std::isfinite(lr[m]) && lr[m] > 0.0, "every lr must be finite and > 0");

    const LstmShape s = lstm_shape(T, d, h1, h2);
    const int b16 = (batch + 15) / 16 * 16;
    LstmArgs g;
    g.s = s;
    g.X = X;
    g.y = y;
    g.n_pad = n_pad;
    g.rows_per_wg = lstm_rows_per_wg(ctx);
    g.theta = theta;
    g.scratch = scratch + AFM_LSTM_MAX_MODELS;
    g.model_scratch = lstm_layout(s, b16).total;
    LstmGradArgs q;
    q.s = s;
    q.X = X;
    q.n_pad = n_pad;
    q.theta = theta;
    q.scratch = g.scratch;
    q.model_scratch = g.model_scratch;
    q.lr = scratch;
    q.c1 = 1.0 - beta1;
    q.c2 = 1.0 - beta2;
    q.eps = eps;
    q.gout = nullptr;
    // lr is a host array the caller may free after the call: a copy from pageable memory has left
    // the caller's buffer when hipMemcpyAsync returns (the runtime may block in it until the
    // stream's earlier work has drained: the one place of the call where the host can wait)
    AFM_HIP(hipMemcpyAsync(scratch, lr, sizeof(double) * M, hipMemcpyHostToDevice, ctx->stream));
    const int64_t head = lstm_layout(s, b16).opart;              // m | v | state
    hipLaunchKernelGGL(lstm_init_kernel, dim3(64, (unsigned)M), dim3(256), 0, ctx->stream, g.scratch,
                       g.model_scratch, head);
    double b1p = 1.0, b2p = 1.0;
    for (int epoch = 0; epoch < epochs; ++epoch) {
        for (int64_t i0 = 0; i0 < n_train; i0 += batch) {
            const int nb = (int)std::min<int64_t>(batch, n_train - i0);
            g.i0 = q.i0 = i0;
            g.n = nb;
            q.nb = nb;
            g.rows16 = q.rows16 = (nb + 15) / 16 * 16;
            g.l = q.l = lstm_layout(s, g.rows16);
            g.out = nullptr;
            g.scale = 2.0 / (double)nb;
            b1p = b1p * beta1;
            b2p = b2p * beta2;
            q.b1p = b1p;
            q.b2p = b2p;
            AFM_HIP(lstm_launch_step(ctx, g, q, M, true));
        }
        // the eval rows through the forward kernel, kLstmParts tiles a launch
        for (int64_t e0 = 0; e0 < n_eval; e0 += kLstmParts * kLstmRows) {
            g.i0 = n_train + e0;
            g.n = std::min<int64_t>(kLstmParts * kLstmRows, n_eval - e0);
            g.out = nullptr;
            AFM_HIP(lstm_launch_forward<kEval>(ctx, g, M));
            hipLaunchKernelGGL(lstm_fold_kernel, dim3((unsigned)M), dim3(64), 0, ctx->stream,
                               g.scratch, g.model_scratch, g.l.ostate, g.l.opart, 1,
                               (int)((g.n + kLstmRows - 1) / kLstmRows));
        }
        hipLaunchKernelGGL(lstm_epoch_kernel, dim3(16, (unsigned)M), dim3(256), 0, ctx->stream,
                           g.scratch, g.model_scratch, g.l.ostate, theta, s.P, evals, snaps, epochs,
                           epoch);
    }
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_lstm_grad_f64(afm_ctx* ctx, const double* X, const double* y, int64_t n_pad,
                                 int64_t i0, int nb, int T, int d, int h1, int h2, int M,
                                 const double* theta, double* grad, double* F, double* scratch) {
    AFM_CTX(ctx);
    AFM_LSTM_CHECK_COMMON(n_pad);
    AFM_CHECK_ARG(nb >= 1 && nb <= AFM_LSTM_MAX_BATCH, "nb must be in 1..1024");
    AFM_CHECK_ARG(i0 >= 0 && i0 <= n_pad && nb <= n_pad - i0, "need i0 >= 0 and i0 + nb <= n_pad");
    AFM_CHECK_ARG(X && y && theta && grad && scratch, "null buffer");
    AFM_CHECK_ARG(lstm_aligned16(X) && lstm_aligned16(y) && lstm_aligned16(theta) &&
                      lstm_aligned16(grad) && lstm_aligned16(F) && lstm_aligned16(scratch),
                  "X, y, theta, grad, F and scratch must be 16-byte aligned");
    const LstmShape s = lstm_shape(T, d, h1, h2);
    LstmArgs g;
    g.s = s;
    g.X = X;
    g.y = y;
    g.n_pad = n_pad;
    g.i0 = i0;
    g.n = nb;
    g.rows16 = (nb + 15) / 16 * 16;
    g.l = lstm_layout(s, g.rows16);
    g.rows_per_wg = lstm_rows_per_wg(ctx);
    g.theta = theta;
    g.scratch = scratch + AFM_LSTM_MAX_MODELS;
    g.model_scratch = g.l.total;
    g.out = F;
    g.scale = 2.0 / (double)nb;
    LstmGradArgs q;
    q.s = s;
    q.l = g.l;
    q.X = X;
    q.n_pad = n_pad;
    q.i0 = i0;
    q.nb = nb;
    q.rows16 = g.rows16;
    q.theta = nullptr;
    q.scratch = g.scratch;
    q.model_scratch = g.model_scratch;
    q.lr = nullptr;
    q.b1p = q.b2p = q.c1 = q.c2 = q.eps = 0.0;
    q.gout = grad;
    AFM_HIP(lstm_launch_step(ctx, g, q, M, false));
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_lstm_forward_f64(afm_ctx* ctx, const double* X, int64_t n_pad, int64_t i0,
                                    int64_t n, int T, int d, int h1, int h2, int M,
                                    const double* theta, double* out) {
    AFM_CTX(ctx);
    AFM_LSTM_CHECK_COMMON(n_pad);
    AFM_CHECK_ARG(i0 >= 0 && n >= 0 && i0 <= n_pad && n <= n_pad - i0,
                  "need i0 >= 0, n >= 0 and i0 + n <= n_pad");
    AFM_CHECK_ARG(X && theta && out, "null buffer");
    AFM_CHECK_ARG(lstm_aligned16(X) && lstm_aligned16(theta) && lstm_aligned16(out),
                  "X, theta and out must be 16-byte aligned");
    if (n == 0) return AFM_OK;
    LstmArgs g;
    g.s = lstm_shape(T, d, h1, h2);
    g.l = lstm_layout(g.s, 16);
    g.X = X;
    g.y = nullptr;
    g.n_pad = n_pad;
    g.i0 = i0;
    g.n = n;
    g.rows16 = 0;
    g.rows_per_wg = lstm_rows_per_wg(ctx);
    g.theta = theta;
    g.scratch = nullptr;
    g.model_scratch = 0;
    g.out = out;
    g.scale = 0.0;
    AFM_HIP(lstm_launch_forward<kPredict>(ctx, g, M));
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_lstm_act_f64(afm_ctx* ctx, int kind, const double* x, int64_t n, double* out) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(kind == 0 || kind == 1, "kind must be 0 (sigmoid) or 1 (tanh)");
    AFM_CHECK_ARG(n >= 0 && n < (1ll << 31), "n must be in 0..2^31");
    AFM_CHECK_ARG(x && out, "null buffer");
    if (n == 0) return AFM_OK;
    hipLaunchKernelGGL(lstm_act_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, kind, x, n, out);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
