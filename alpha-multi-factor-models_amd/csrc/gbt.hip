// Gradient-boosted regression trees (include/afm_gbt.h): values / bins of the design, one level's
// gradient histograms, the whole fit (no host synchronisation inside) and the tree walk over the
// panel.  Gradients are fixed-point int64, so every histogram sum is exact and independent of the
// order of addition; the only atomics are integer adds and an integer max.
#include "afm_internal.h"

#include <algorithm>

#include "afm_gbt.h"

namespace {

using u64 = unsigned long long;
using i64 = long long;

constexpr int kLdsBins = 256;          // bin stride of the LDS histogram (a bin is a byte)
constexpr int kHistSlots = 4096;       // LDS slots of a workgroup: 16 (node, column) pairs
constexpr int kPairs = kHistSlots / kLdsBins;
constexpr int kMomBlocks = 256;        // the fixed row partition of the moments
constexpr int64_t kMaxChunk = 1 << 20; // rows of a chunk: sum w of a slot stays below 2^32

// state of a fit on the device
struct GbtCtl {
    u64 gmax_bits;   // max |g| over w > 0 as its bit pattern (integer max); 0 between rounds
    i64 W;           // sum w
    int e;           // the round's scale exponent
    int pad;
};

struct GbtCand {     // best split of a (node, column): b < 0 = none
    double gain;
    i64 b, GL, HL;
};

__device__ inline double pow2(int e) { return __longlong_as_double((i64)(1023 + e) << 52); }

__device__ inline int scale_exponent(u64 gmax_bits, i64 W) {
    if (gmax_bits == 0) return 0;
    const int E = (int)(gmax_bits >> 52) - 1022;          // frexp's exponent (subnormal: clamped)
    const int e = 62 - (64 - __clzll(W)) - E;
    return e > 960 ? 960 : e;
}

__device__ inline double node_value(i64 G, i64 H, int e, double eta, double lam) {
    return eta * (-((double)G * pow2(-e)) / ((double)H + lam));
}

__device__ inline double row_value(const double* plane, const double* zs, int k, int64_t lda,
                                   const int32_t* rows_t, const int32_t* rows_a, int64_t i) {
    const int64_t t = rows_t ? rows_t[i] : 0, a = rows_a ? rows_a[i] : i;
    double x = plane[t * lda + a];
    if (zs) {
        const double2 m = reinterpret_cast<const double2*>(zs)[(int64_t)k * lda + a];
        x = (x - m.x) * m.y;
    }
    return x;
}

__global__ __launch_bounds__(256) void gbt_values_kernel(
    const double* base, int64_t col_stride, int64_t lda, const int32_t* cols, int k,
    const double* zs, const int32_t* rows_t, const int32_t* rows_a, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = row_value(base + (int64_t)cols[k] * col_stride, zs, k, lda, rows_t, rows_a, i);
}

// 16 rows of one column per thread: their bins leave in one 16-byte store.
__global__ __launch_bounds__(256) void gbt_bin_kernel(
    const double* base, int64_t col_stride, int64_t lda, const int32_t* cols, const double* zs,
    const int32_t* rows_t, const int32_t* rows_a, int64_t n, int64_t n_pad, const double* cuts,
    const int32_t* ncuts, int B, uint8_t* bins) {
    __shared__ double sc[kLdsBins];
    const int k = blockIdx.y;
    int nc = ncuts[k];
    nc = nc < 0 ? 0 : (nc > B - 1 ? B - 1 : nc);
    for (int j = threadIdx.x; j < nc; j += 256) sc[j] = cuts[(int64_t)k * (B - 1) + j];
    __syncthreads();
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i0 >= n_pad) return;                      // n_pad % 16 == 0: a group is whole or absent
    const double* plane = base + (int64_t)cols[k] * col_stride;
    uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t i = i0 + r;
        uint32_t b = 0;
        if (i < n) {
            const double x = row_value(plane, zs, k, lda, rows_t, rows_a, i);
            int lo = 0, hi = nc;
            while (lo < hi) {                     // the number of cuts <= x
                const int mid = (lo + hi) >> 1;
                if (sc[mid] <= x) lo = mid + 1; else hi = mid;
            }
            b = (uint32_t)lo;
        }
        pk[r >> 2] |= b << (8 * (r & 3));
    }
    *reinterpret_cast<uint4*>(bins + (int64_t)k * n_pad + i0) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

// One level's histograms.  Workgroup (x, y): the row chunk x, the column tile y % ntiles (ct
// columns) and the node group y / ntiles (nn nodes); LDS [node][column][256] of {u64 sum q, u32
// sum w}, ds_add_u64 / ds_add_u32; non-zero slots are added into hist (zeroed by the caller) with
// 64-bit integer atomics.  A thread takes 4 consecutive rows: one 4-byte load of their bins per
// column, 16-byte loads of node / q / w.
__global__ __launch_bounds__(256) void gbt_hist_kernel(
    const uint8_t* bins, int64_t n, int64_t n_pad, int p, int B, const int32_t* node, const i64* q,
    const int32_t* w, int nnodes, int ct, int nn, int ntiles, int64_t rows_per_wg, u64* hist) {
    __shared__ u64 sq[kHistSlots];
    __shared__ uint32_t sw[kHistSlots];
    const int tid = threadIdx.x;
    const int tile = (int)(blockIdx.y % (unsigned)ntiles), grp = (int)(blockIdx.y / (unsigned)ntiles);
    const int c0 = tile * ct, nc = min(ct, p - c0);
    const int n0 = grp * nn, nloc = min(nn, nnodes - n0);
    const int used = nloc * ct * kLdsBins;                  // <= kHistSlots: nn * ct <= kPairs
    for (int j = tid; j < used; j += 256) {
        sq[j] = 0;
        sw[j] = 0;
    }
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;   // a multiple of 4
    const int64_t r1 = min(n, r0 + rows_per_wg);
    for (int64_t i0 = r0 + (int64_t)tid * 4; i0 < r1; i0 += 1024) {
        int loc[4], ww[4];
        i64 qq[4];
        if (i0 + 4 <= r1) {
            const int4 nd = *reinterpret_cast<const int4*>(node + i0);
            const int4 wv = *reinterpret_cast<const int4*>(w + i0);
            const longlong2 qa = *reinterpret_cast<const longlong2*>(q + i0);
            const longlong2 qb = *reinterpret_cast<const longlong2*>(q + i0 + 2);
            loc[0] = nd.x; loc[1] = nd.y; loc[2] = nd.z; loc[3] = nd.w;
            ww[0] = wv.x; ww[1] = wv.y; ww[2] = wv.z; ww[3] = wv.w;
            qq[0] = qa.x; qq[1] = qa.y; qq[2] = qb.x; qq[3] = qb.y;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = i0 + r < r1;
                loc[r] = in ? node[i0 + r] : -1;
                ww[r] = in ? w[i0 + r] : 0;
                qq[r] = in ? q[i0 + r] : 0;
            }
        }
        bool any = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = loc[r] - n0;
            const bool use = loc[r] >= 0 && l >= 0 && l < nloc && (qq[r] != 0 || ww[r] != 0);
            loc[r] = use ? l * ct : -1;                     // (node, column 0) pair, or unused
            any |= use;
        }
        if (!any) continue;
        for (int c = 0; c < nc; ++c) {
            // i0 + 3 < n_pad: i0 < n <= n_pad, both multiples of 4
            const uint32_t bw = *reinterpret_cast<const uint32_t*>(bins + (int64_t)(c0 + c) * n_pad + i0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (loc[r] < 0) continue;
                const int slot = (loc[r] + c) * kLdsBins + (int)((bw >> (8 * r)) & 255u);
                atomicAdd(&sq[slot], (u64)qq[r]);
                atomicAdd(&sw[slot], (uint32_t)ww[r]);
            }
        }
    }
    __syncthreads();
    for (int j = tid; j < used; j += 256) {
        const int b = j & (kLdsBins - 1), pair = j >> 8;
        const int c = pair % ct, l = pair / ct;
        if (b >= B || c >= nc) continue;
        const u64 vq = sq[j];
        const uint32_t vw = sw[j];
        if (vq == 0 && vw == 0) continue;
        u64* h = hist + ((((int64_t)(n0 + l) * p + (c0 + c)) * B + b) << 1);
        if (vq) atomicAdd(h, vq);
        if (vw) atomicAdd(h + 1, (u64)vw);
    }
}

// ---- the fit's small kernels ----------------------------------------------------------------

__global__ __launch_bounds__(256) void gbt_wsum_kernel(const int32_t* w, int64_t n, GbtCtl* ctl) {
    __shared__ i64 s[256];
    i64 a = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        a += w[i] > 0 ? w[i] : 0;
    s[threadIdx.x] = a;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s[0]) atomicAdd(reinterpret_cast<u64*>(&ctl->W), (u64)s[0]);
}

__global__ __launch_bounds__(256) void gbt_gmax_kernel(const double* F, const double* y,
                                                       const int32_t* w, int64_t n, GbtCtl* ctl) {
    __shared__ u64 s[256];
    u64 m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        if (w[i] > 0) {
            const u64 b = (u64)__double_as_longlong(fabs(F[i] - y[i]));
            m = b > m ? b : m;
        }
    s[threadIdx.x] = m;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st && s[threadIdx.x + st] > s[threadIdx.x])
            s[threadIdx.x] = s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s[0]) atomicMax(&ctl->gmax_bits, s[0]);
}

// q = w * rint(g * 2^e); every row starts the tree at the root.
__global__ __launch_bounds__(256) void gbt_quantize_kernel(const double* F, const double* y,
                                                           const int32_t* w, int64_t n,
                                                           GbtCtl* ctl, i64* q, int32_t* node) {
    const int e = scale_exponent(ctl->gmax_bits, ctl->W);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) ctl->e = e;
    if (i >= n) return;
    const int wi = w[i];
    q[i] = wi > 0 ? (i64)wi * (i64)rint((F[i] - y[i]) * pow2(e)) : 0;
    node[i] = 0;
}

// The round's tree starts empty; the root's sums are those of column 0's bins of the level-0
// histogram (every row has one bin there).
__global__ __launch_bounds__(256) void gbt_root_kernel(const i64* hist, int B, int nn_tree,
                                                       const GbtCtl* ctl, double eta, double lam,
                                                       i64* nstat, int32_t* feat, int32_t* bin,
                                                       double* thr, double* val) {
    __shared__ i64 sg[256], sh[256];
    const int tid = threadIdx.x;
    for (int v = 1 + tid; v < nn_tree; v += 256) {
        feat[v] = -2;
        bin[v] = -1;
        thr[v] = 0.0;
        val[v] = 0.0;
    }
    sg[tid] = tid < B ? hist[2 * tid] : 0;
    sh[tid] = tid < B ? hist[2 * tid + 1] : 0;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            sg[tid] += sg[tid + st];
            sh[tid] += sh[tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        nstat[0] = sg[0];
        nstat[1] = sh[0];
        feat[0] = -1;
        bin[0] = -1;
        thr[0] = 0.0;
        val[0] = node_value(sg[0], sh[0], ctl->e, eta, lam);
    }
}

__device__ inline i64 shfl_up_i64(i64 v, int d) { return __shfl_up(v, d); }

// One wave per (column, node of the level): prefix sums of the bins (4 per lane), the gain of
// every candidate, the best one (largest gain, then lowest b).
__global__ __launch_bounds__(64) void gbt_scan_kernel(
    const i64* hist, int p, int B, int first, const int32_t* feat, const i64* nstat,
    const int32_t* ncuts, const GbtCtl* ctl, double lam, double gamma, double mcw, GbtCand* cand) {
    const int k = blockIdx.x, j = blockIdx.y, v = first + j, lane = threadIdx.x;
    GbtCand* out = cand + (int64_t)j * p + k;
    int nc = ncuts[k];
    nc = nc > B - 1 ? B - 1 : nc;
    if (feat[v] != -1 || nc <= 0) {
        if (lane == 0) out->b = -1;
        return;
    }
    const i64* h = hist + ((int64_t)j * p + k) * B * 2;
    i64 lq[4], lw[4], sq = 0, sw = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = lane * 4 + r;
        if (b < B) {
            sq += h[2 * b];
            sw += h[2 * b + 1];
        }
        lq[r] = sq;
        lw[r] = sw;
    }
    i64 pq = sq, pw = sw;                                  // inclusive scan over the lanes
    for (int off = 1; off < 64; off <<= 1) {
        const i64 tq = shfl_up_i64(pq, off), tw = shfl_up_i64(pw, off);
        if (lane >= off) {
            pq += tq;
            pw += tw;
        }
    }
    const i64 exq = pq - sq, exw = pw - sw;
    const i64 G = nstat[2 * v], H = nstat[2 * v + 1];
    const double inv = pow2(-ctl->e);
    const double g = (double)G * inv;
    const double gp = g * g / ((double)H + lam);
    double bg = 0.0;
    i64 bb = -1, bGL = 0, bHL = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = lane * 4 + r;
        if (b >= nc) continue;
        const i64 GL = exq + lq[r], HL = exw + lw[r], HR = H - HL;
        const double gl = (double)GL * inv, gr = (double)(G - GL) * inv;
        const double gain = gl * gl / ((double)HL + lam) + gr * gr / ((double)HR + lam) - gp;
        if ((double)HL >= mcw && (double)HR >= mcw && gain > gamma && (bb < 0 || gain > bg)) {
            bg = gain;
            bb = b;
            bGL = GL;
            bHL = HL;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double og = __shfl_xor(bg, off);
        const i64 ob = __shfl_xor(bb, off), oGL = __shfl_xor(bGL, off), oHL = __shfl_xor(bHL, off);
        if (ob >= 0 && (bb < 0 || og > bg || (og == bg && ob < bb))) {
            bg = og;
            bb = ob;
            bGL = oGL;
            bHL = oHL;
        }
    }
    if (lane == 0) {
        out->gain = bg;
        out->b = bb;
        out->GL = bGL;
        out->HL = bHL;
    }
}

// One workgroup per node of the level: the best column (largest gain, then lowest k); a split
// writes the node and makes its children leaves with their sums and values.
__global__ __launch_bounds__(256) void gbt_pick_kernel(
    const GbtCand* cand, int p, int B, int first, const double* cuts, const GbtCtl* ctl, double eta,
    double lam, i64* nstat, int32_t* feat, int32_t* bin, double* thr, double* val) {
    __shared__ double sg[256];
    __shared__ int sk[256];
    const int j = blockIdx.x, v = first + j, tid = threadIdx.x;
    if (feat[v] != -1) return;
    const GbtCand* row = cand + (int64_t)j * p;
    const bool has = tid < p && row[tid].b >= 0;
    sg[tid] = has ? row[tid].gain : 0.0;
    sk[tid] = has ? tid : -1;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            const int ok = sk[tid + st];
            const double og = sg[tid + st];
            if (ok >= 0 && (sk[tid] < 0 || og > sg[tid] || (og == sg[tid] && ok < sk[tid]))) {
                sk[tid] = ok;
                sg[tid] = og;
            }
        }
        __syncthreads();
    }
    if (tid != 0 || sk[0] < 0) return;
    const int k = sk[0];
    const GbtCand c = row[k];
    const i64 G = nstat[2 * v], H = nstat[2 * v + 1];
    const int e = ctl->e;
    feat[v] = k;
    bin[v] = (int)c.b;
    thr[v] = cuts[(int64_t)k * (B - 1) + c.b];
    const int L = 2 * v + 1, R = 2 * v + 2;
    nstat[2 * L] = c.GL;
    nstat[2 * L + 1] = c.HL;
    nstat[2 * R] = G - c.GL;
    nstat[2 * R + 1] = H - c.HL;
    feat[L] = -1;
    feat[R] = -1;
    val[L] = node_value(c.GL, c.HL, e, eta, lam);
    val[R] = node_value(G - c.GL, H - c.HL, e, eta, lam);
}

// Rows of the level's nodes move to a child (level-local index) or settle in their leaf.
__global__ __launch_bounds__(256) void gbt_route_kernel(const uint8_t* bins, int64_t n,
                                                        int64_t n_pad, int first,
                                                        const int32_t* feat, const int32_t* bin,
                                                        int32_t* node, int32_t* leaf) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = node[i];
    if (j < 0) return;
    const int v = first + j, k = feat[v];
    if (k >= 0) {
        node[i] = 2 * j + (bins[(int64_t)k * n_pad + i] > (unsigned)bin[v] ? 1 : 0);
    } else {
        leaf[i] = v;
        node[i] = -1;
    }
}

// F += val[leaf], and the block's share of the twelve moments: thread t of block b takes the rows
// (b * 256 + t) + j * 65536 in order, then a fixed tree over the block.
__global__ __launch_bounds__(256) void gbt_update_kernel(
    int64_t n, int last_first, const int32_t* node, const int32_t* leaf, const double* val,
    const double* y, const int32_t* w, double* F, GbtCtl* ctl, double* part) {
    __shared__ double s[12][256];
    const int tid = threadIdx.x;
    double m[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) m[c] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)kMomBlocks * 256) {
        const int nd = node[i];
        const int v = nd >= 0 ? last_first + nd : leaf[i];
        const double f = F[i] + val[v], yy = y[i];
        F[i] = f;
        const double t3 = f * f, t4 = yy * yy, t5 = f * yy;
        if (w[i] > 0) {
            m[0] += 1.0; m[1] += f; m[2] += yy; m[3] += t3; m[4] += t4; m[5] += t5;
        } else {
            m[6] += 1.0; m[7] += f; m[8] += yy; m[9] += t3; m[10] += t4; m[11] += t5;
        }
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) s[c][tid] = m[c];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st)
#pragma unroll
            for (int c = 0; c < 12; ++c) s[c][tid] += s[c][tid + st];
        __syncthreads();
    }
    if (tid < 12) part[blockIdx.x * 12 + tid] = s[tid][0];
    if (blockIdx.x == 0 && tid == 0) ctl->gmax_bits = 0;    // the next round's max starts from 0
}

__global__ __launch_bounds__(256) void gbt_moments_kernel(const double* part, double* evals) {
    __shared__ double s[12][256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 12; ++c) s[c][tid] = part[tid * 12 + c];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st)
#pragma unroll
            for (int c = 0; c < 12; ++c) s[c][tid] += s[c][tid + st];
        __syncthreads();
    }
    if (tid < 12) evals[tid] = s[tid][0];
}

// One thread per cell, 4 dates x 64 assets per workgroup (zpredict_kernel's shape).
__global__ __launch_bounds__(256) void gbt_predict_kernel(
    const double* base, int64_t col_stride, int64_t lda, int64_t t0, int64_t nt,
    const int32_t* cols, int p, const double* zs, const int32_t* feat, const double* thr,
    const double* val, int depth, int n_trees, double base_score, const uint64_t* bits,
    double* pred) {
    const int tid = threadIdx.x;
    const int64_t a = (int64_t)blockIdx.x * 64 + (tid & 63);
    const int64_t t = t0 + (int64_t)blockIdx.y * 4 + (tid >> 6);
    if (t >= t0 + nt) return;
    const bool use = (bits[(t >> 6) * lda + a] >> (t & 63)) & 1ull;
    double s = __builtin_nan("");
    if (use) {
        s = base_score;
        const double* cell = base + t * lda + a;
        const int nn = (2 << depth) - 1;
        for (int r = 0; r < n_trees; ++r) {
            const int32_t* f = feat + (int64_t)r * nn;
            const double* th = thr + (int64_t)r * nn;
            int v = 0;
            for (int d = 0; d < depth; ++d) {
                const int k = f[v];
                if (k < 0 || k >= p) break;
                double x = cell[(int64_t)cols[k] * col_stride];
                if (zs) {
                    const double2 m = reinterpret_cast<const double2*>(zs)[(int64_t)k * lda + a];
                    x = (x - m.x) * m.y;
                }
                v = x < th[v] ? 2 * v + 1 : 2 * v + 2;
            }
            s = s + val[(int64_t)r * nn + v];
        }
    }
    pred[t * lda + a] = s;
}

inline int64_t up256(int64_t b) { return (b + 255) / 256 * 256; }

struct GbtScratch {
    int64_t hist, cand, nstat, ctl, node, leaf, q, part, total;
};

GbtScratch gbt_layout(int64_t n, int p, int D, int B) {
    GbtScratch s;
    const int64_t lvl = (int64_t)1 << (D - 1), nn = ((int64_t)2 << D) - 1;
    int64_t o = 0;
    s.hist = o;  o += up256(lvl * p * B * 16);
    s.cand = o;  o += up256(lvl * p * (int64_t)sizeof(GbtCand));
    s.nstat = o; o += up256(nn * 16);
    s.ctl = o;   o += up256(sizeof(GbtCtl));
    s.node = o;  o += up256(n * 4);
    s.leaf = o;  o += up256(n * 4);
    s.q = o;     o += up256(n * 8);
    s.part = o;  o += up256(kMomBlocks * 12 * 8);
    s.total = o;
    return s;
}

const char* gbt_shape_error(int64_t n, int p, int D, int B) {
    if (n < 1 || n >= ((int64_t)1 << 31)) return "need 1 <= n < 2^31";
    if (p < 1 || p > AFM_GBT_MAX_COLS) return "need 1 <= p <= 256";
    if (D < 1 || D > AFM_GBT_MAX_DEPTH) return "need 1 <= max_depth <= 6";
    if (B < 2 || B > AFM_GBT_MAX_BIN) return "need 2 <= max_bin <= 256";
    return nullptr;
}

inline bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

// hist of one level: zeroed, then the chunks x tiles x node groups of gbt_hist_kernel
hipError_t hist_level(afm_ctx* ctx, int64_t rows_opt, const uint8_t* bins, int64_t n, int64_t n_pad,
                      int p, int B, const int32_t* node, const i64* q, const int32_t* w, int nnodes,
                      u64* hist) {
    hipError_t err = hipMemsetAsync(hist, 0, (size_t)nnodes * p * B * 16, ctx->stream);
    if (err != hipSuccess) return err;
    const int nn = nnodes < kPairs ? nnodes : kPairs, ct = kPairs / nn;
    const int ntiles = (p + ct - 1) / ct, ngroups = (nnodes + nn - 1) / nn;
    int64_t rows = rows_opt;
    if (rows <= 0) {    // about 18 workgroups per CU (3 are resident: 6 rounds), chunks of >= 1024 rows
        const int64_t target = std::max<int64_t>(1, (18 * (int64_t)afm_ctx_cus(ctx)) / (ntiles * ngroups));
        rows = std::max<int64_t>(1024, (n + target - 1) / target);
    }
    rows = std::min<int64_t>((rows + 3) / 4 * 4, kMaxChunk);
    const int64_t nchunks = (n + rows - 1) / rows;
    hipLaunchKernelGGL(gbt_hist_kernel, dim3((unsigned)nchunks, (unsigned)(ntiles * ngroups)),
                       dim3(256), 0, ctx->stream, bins, n, n_pad, p, B, node, q, w, nnodes, ct, nn,
                       ntiles, rows, hist);
    return hipGetLastError();
}

}  // namespace

extern "C" int64_t afm_gbt_scratch_bytes(int64_t n, int p, int max_depth, int max_bin) {
    if (const char* msg = gbt_shape_error(n, p, max_depth, max_bin)) {
        afm_set_error(std::string("afm_gbt_scratch_bytes: ") + msg);
        return AFM_E_ARG;
    }
    return gbt_layout(n, p, max_depth, max_bin).total;
}

extern "C" int afm_gbt_values_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                                  int64_t lda, const int32_t* cols, int k, const double* zs,
                                  const int32_t* rows_t, const int32_t* rows_a, int64_t n,
                                  double* out) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(base && cols && out, "null buffer");
    AFM_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "need 1 <= n < 2^31");
    AFM_CHECK_ARG(T >= 1 && lda >= 1 && lda % 64 == 0 && k >= 0 && k < AFM_GBT_MAX_COLS,
                  "bad shape");
    hipLaunchKernelGGL(gbt_values_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, base, col_stride, lda, cols, k, zs, rows_t, rows_a, n, out);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_gbt_bin_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                               int64_t lda, const int32_t* cols, int p, const double* zs,
                               const int32_t* rows_t, const int32_t* rows_a, int64_t n,
                               int64_t n_pad, const double* cuts, const int32_t* ncuts,
                               int max_bin, uint8_t* bins) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(base && cols && cuts && ncuts && bins, "null buffer");
    if (const char* msg = gbt_shape_error(n, p, 1, max_bin)) AFM_CHECK_ARG(false, msg);
    AFM_CHECK_ARG(T >= 1 && lda >= 1 && lda % 64 == 0, "bad shape");
    AFM_CHECK_ARG(n_pad >= n && n_pad % 64 == 0, "n_pad: a multiple of 64 >= n");
    AFM_CHECK_ARG(aligned16(bins), "bins must be 16-byte aligned");
    hipLaunchKernelGGL(gbt_bin_kernel, dim3((unsigned)((n_pad + 4095) / 4096), (unsigned)p),
                       dim3(256), 0, ctx->stream, base, col_stride, lda, cols, zs, rows_t, rows_a,
                       n, n_pad, cuts, ncuts, max_bin, bins);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int afm_gbt_hist_i64(afm_ctx* ctx, const uint8_t* bins, int64_t n, int64_t n_pad, int p,
                                int max_bin, const int32_t* node, const int64_t* q,
                                const int32_t* w, int nnodes, int64_t* hist) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(bins && node && q && w && hist, "null buffer");
    if (const char* msg = gbt_shape_error(n, p, 1, max_bin)) AFM_CHECK_ARG(false, msg);
    AFM_CHECK_ARG(n_pad >= n && n_pad % 64 == 0, "n_pad: a multiple of 64 >= n");
    AFM_CHECK_ARG(nnodes >= 1 && nnodes <= 32, "need 1 <= nnodes <= 32");
    AFM_CHECK_ARG(aligned16(bins) && aligned16(node) && aligned16(q) && aligned16(w),
                  "bins, node, q and w must be 16-byte aligned");
    AFM_HIP(hist_level(ctx, ctx->gbt_rows_per_wg, bins, n, n_pad, p, max_bin, node,
                       reinterpret_cast<const i64*>(q), w, nnodes, reinterpret_cast<u64*>(hist)));
    return AFM_OK;
}

extern "C" int afm_gbt_fit_f64(afm_ctx* ctx, const uint8_t* bins, int64_t n, int64_t n_pad, int p,
                               const double* cuts, const int32_t* ncuts, const double* y,
                               const int32_t* w, int n_rounds, int max_depth, int max_bin,
                               double eta, double reg_lambda, double gamma,
                               double min_child_weight, int32_t* feat, int32_t* bin, double* thr,
                               double* val, double* F, double* evals, uint64_t* scratch) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(bins && cuts && ncuts && y && w && feat && bin && thr && val && F && evals &&
                      scratch, "null buffer");
    if (const char* msg = gbt_shape_error(n, p, max_depth, max_bin)) AFM_CHECK_ARG(false, msg);
    AFM_CHECK_ARG(n_pad >= n && n_pad % 64 == 0, "n_pad: a multiple of 64 >= n");
    AFM_CHECK_ARG(n_rounds >= 1, "need n_rounds >= 1");
    AFM_CHECK_ARG(min_child_weight >= 1.0, "need min_child_weight >= 1");
    AFM_CHECK_ARG(reg_lambda >= 0.0 && gamma >= 0.0, "need reg_lambda >= 0 and gamma >= 0");
    AFM_CHECK_ARG(aligned16(bins) && aligned16(w) && aligned16(scratch),
                  "bins, w and scratch must be 16-byte aligned");
    const GbtScratch L = gbt_layout(n, p, max_depth, max_bin);
    char* sb = reinterpret_cast<char*>(scratch);
    u64* hist = reinterpret_cast<u64*>(sb + L.hist);
    GbtCand* cand = reinterpret_cast<GbtCand*>(sb + L.cand);
    i64* nstat = reinterpret_cast<i64*>(sb + L.nstat);
    GbtCtl* ctl = reinterpret_cast<GbtCtl*>(sb + L.ctl);
    int32_t* node = reinterpret_cast<int32_t*>(sb + L.node);
    int32_t* leaf = reinterpret_cast<int32_t*>(sb + L.leaf);
    i64* q = reinterpret_cast<i64*>(sb + L.q);
    double* part = reinterpret_cast<double*>(sb + L.part);
    hipStream_t st = ctx->stream;
    const int nn_tree = (2 << max_depth) - 1;
    const unsigned rowgrid = (unsigned)((n + 255) / 256);
    const unsigned redgrid = (unsigned)std::min<int64_t>(rowgrid, 1024);
    const int64_t rows_opt = ctx->gbt_rows_per_wg;
    AFM_HIP(hipMemsetAsync(ctl, 0, sizeof(GbtCtl), st));
    hipLaunchKernelGGL(gbt_wsum_kernel, dim3(redgrid), dim3(256), 0, st, w, n, ctl);
    for (int r = 0; r < n_rounds; ++r) {
        int32_t* tf = feat + (int64_t)r * nn_tree;
        int32_t* tb = bin + (int64_t)r * nn_tree;
        double* tt = thr + (int64_t)r * nn_tree;
        double* tv = val + (int64_t)r * nn_tree;
        hipLaunchKernelGGL(gbt_gmax_kernel, dim3(redgrid), dim3(256), 0, st, F, y, w, n, ctl);
        hipLaunchKernelGGL(gbt_quantize_kernel, dim3(rowgrid), dim3(256), 0, st, F, y, w, n, ctl, q,
                           node);
        for (int d = 0; d < max_depth; ++d) {
            const int nnodes = 1 << d, first = nnodes - 1;
            AFM_HIP(hist_level(ctx, rows_opt, bins, n, n_pad, p, max_bin, node, q, w, nnodes, hist));
            if (d == 0)
                hipLaunchKernelGGL(gbt_root_kernel, dim3(1), dim3(256), 0, st,
                                   reinterpret_cast<const i64*>(hist), max_bin, nn_tree, ctl, eta,
                                   reg_lambda, nstat, tf, tb, tt, tv);
            hipLaunchKernelGGL(gbt_scan_kernel, dim3((unsigned)p, (unsigned)nnodes), dim3(64), 0, st,
                               reinterpret_cast<const i64*>(hist), p, max_bin, first, tf, nstat,
                               ncuts, ctl, reg_lambda, gamma, min_child_weight, cand);
            hipLaunchKernelGGL(gbt_pick_kernel, dim3((unsigned)nnodes), dim3(256), 0, st, cand, p,
                               max_bin, first, cuts, ctl, eta, reg_lambda, nstat, tf, tb, tt, tv);
            hipLaunchKernelGGL(gbt_route_kernel, dim3(rowgrid), dim3(256), 0, st, bins, n, n_pad,
                               first, tf, tb, node, leaf);
        }
        hipLaunchKernelGGL(gbt_update_kernel, dim3(kMomBlocks), dim3(256), 0, st, n,
                           (1 << max_depth) - 1, node, leaf, tv, y, w, F, ctl, part);
        hipLaunchKernelGGL(gbt_moments_kernel, dim3(1), dim3(256), 0, st, part,
                           evals + (int64_t)r * 12);
        AFM_HIP(hipGetLastError());
    }
    return AFM_OK;
}

extern "C" int afm_gbt_predict_f64(afm_ctx* ctx, const double* base, int64_t col_stride,
                                   int64_t lda, int64_t t0, int64_t nt, const int32_t* cols, int p,
                                   const double* zs, const int32_t* feat, const double* thr,
                                   const double* val, int max_depth, int n_trees,
                                   double base_score, const uint64_t* bits, double* pred) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(base && cols && feat && thr && val && bits && pred, "null buffer");
    AFM_CHECK_ARG(lda >= 64 && lda % 64 == 0 && nt >= 0 && t0 >= 0, "bad shape");
    AFM_CHECK_ARG(p >= 1 && p <= AFM_GBT_MAX_COLS, "need 1 <= p <= 256");
    AFM_CHECK_ARG(max_depth >= 1 && max_depth <= AFM_GBT_MAX_DEPTH, "need 1 <= max_depth <= 6");
    AFM_CHECK_ARG(n_trees >= 0, "need n_trees >= 0");
    if (nt == 0) return AFM_OK;
    dim3 grid((unsigned)(lda / 64), (unsigned)((nt + 3) / 4));
    hipLaunchKernelGGL(gbt_predict_kernel, grid, dim3(256), 0, ctx->stream, base, col_stride, lda,
                       t0, nt, cols, p, zs, feat, thr, val, max_depth, n_trees, base_score, bits,
                       pred);
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}
