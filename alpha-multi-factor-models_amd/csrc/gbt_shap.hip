// Attribution of the boosted trees (include/afm_gbt_shap.h): the cover of every node, and the exact
// path-dependent TreeSHAP contributions in the closed per-path form -- one lane per cell, scalar
// fp64, every operation in the header's order.  The only atomics are integer adds.
#include "afm_internal.h"

#include <algorithm>
#include <type_traits>

#include "afm_gbt_shap.h"

namespace {

using u64 = unsigned long long;
using i64 = long long;

constexpr int kMaxD = AFM_GBT_MAX_DEPTH;
constexpr int kMaxNodes = (2 << kMaxD) - 1;   // 127
constexpr int kCovTrees = 32;                 // trees of a cover slab: 32 x 127 x 12 B = 48 KB of LDS
constexpr int64_t kCovMaxChunk = 1 << 20;     // rows of a chunk: a node's sum w stays below 2^32

// ---- cover ------------------------------------------------------------------------------------

// Workgroup (x, y): the row chunk x and the trees [32 y, 32 y + 32).  The slab's feat / bin and
// one u32 counter per node live in LDS; a thread walks its rows down every tree of the slab and
// counts each row once, at the node where it settles (ds_add_u32); a split's count is then the sum
// of its children's, level by level from the bottom -- integers, so the same cover as counting at
// every node.  Non-zero counters are added into cover (zeroed by the caller) with 64-bit integer
// atomics.
__global__ __launch_bounds__(256) void gbt_cover_kernel(
    const uint8_t* bins, int64_t n, int64_t n_pad, int p, const int32_t* w, const int32_t* feat,
    const int32_t* bin, int depth, int n_trees, int64_t rows_per_wg, u64* cover) {
    __shared__ int32_t sf[kCovTrees * kMaxNodes];
    __shared__ int32_t sb[kCovTrees * kMaxNodes];
    __shared__ uint32_t sc[kCovTrees * kMaxNodes];
    const int tid = threadIdx.x;
    const int nn = (2 << depth) - 1;
    const int r0 = (int)blockIdx.y * kCovTrees, nt = min(kCovTrees, n_trees - r0);
    const int used = nt * nn;                                  // <= kCovTrees * kMaxNodes
    for (int j = tid; j < used; j += 256) {
        sf[j] = feat[(int64_t)r0 * nn + j];
        sb[j] = bin[(int64_t)r0 * nn + j];
        sc[j] = 0;
    }
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t i1 = min(n, i0 + rows_per_wg);
    for (int64_t i = i0 + tid; i < i1; i += 256) {
        const int wi = w[i];
        if (wi <= 0) continue;
        for (int r = 0; r < nt; ++r) {
            const int o = r * nn;
            int v = 0;                                         // v < nn: at most depth steps down
            for (int d = 0; d < depth; ++d) {
                const int k = sf[o + v];
                if (k < 0 || k >= p) break;
                v = 2 * v + 1 + (bins[(int64_t)k * n_pad + i] > (unsigned)sb[o + v] ? 1 : 0);
            }
            atomicAdd(&sc[o + v], (uint32_t)wi);
        }
    }
    __syncthreads();
    for (int lvl = depth - 1; lvl >= 0; --lvl) {
        const int first = (1 << lvl) - 1, width = 1 << lvl;
        for (int j = tid; j < nt * width; j += 256) {
            const int o = (j >> lvl) * nn, v = first + (j & (width - 1));
            const int k = sf[o + v];
            if (k >= 0 && k < p) sc[o + v] = sc[o + 2 * v + 1] + sc[o + 2 * v + 2];
        }
        __syncthreads();
    }
    for (int j = tid; j < used; j += 256) {
        const uint32_t c = sc[j];
        if (c) atomicAdd(cover + (int64_t)r0 * nn + j, (u64)c);
    }
}

// ---- contributions ----------------------------------------------------------------------------

// One leaf's path, merged by column (afm_gbt_shap.h): what gbt_shap_path_kernel writes and every
// wave of gbt_shap_kernel reads (through LDS), the same in every lane.  Bit v of mask[j] / want[j]: node v splits
// on col[j] / the path goes left there.
struct ShapLeaf {
    double val, bias;              // val[l]; val[l] * prod z
    double z[kMaxD];
    u64 mask[kMaxD], want[kMaxD];
    int32_t col[kMaxD];
    int32_t m, pad;
};
static_assert(sizeof(ShapLeaf) == 192, "ShapLeaf layout");
constexpr int kShapChunk = 8;                  // records staged in LDS at a time (a depth-3 tree)
constexpr int kShapChunkBytes = kShapChunk * (int)sizeof(ShapLeaf);        // 1,536: <= 2 x 1,024

inline int64_t up256(int64_t b) { return (b + 255) / 256 * 256; }

struct ShapScratch {
    int64_t leaves, nleaf, part, cpart, total;
};

ShapScratch shap_layout(int64_t lda, int64_t nt, int p, int D, int n_trees) {
    ShapScratch s;
    const int64_t nblk = lda / 64;
    int64_t o = 0;
    s.leaves = o; o += up256((int64_t)n_trees * ((int64_t)1 << D) * (int64_t)sizeof(ShapLeaf));
    s.nleaf = o;  o += up256((int64_t)n_trees * 4);
    s.part = o;   o += up256(nt * nblk * (p + 1) * 16);
    s.cpart = o;  o += up256(nt * nblk * 8);
    s.total = o;
    return s;
}

// One thread per tree: its leaves in heap order, each with its merged path.  A leaf below a node
// that does not split (a malformed tree) is left out.
__global__ __launch_bounds__(64) void gbt_shap_path_kernel(const int32_t* feat, const double* val,
                                                           const i64* cover, int p, int depth,
                                                           int n_trees, ShapLeaf* leaves,
                                                           int32_t* nleaf) {
    const int r = (int)blockIdx.x * 64 + threadIdx.x;
    if (r >= n_trees) return;
    const int nn = (2 << depth) - 1;
    const int32_t* f = feat + (int64_t)r * nn;
    const double* vl = val + (int64_t)r * nn;
    const i64* cv = cover + (int64_t)r * nn;
    ShapLeaf* out = leaves + ((int64_t)r << depth);
    int cnt = 0;
    for (int v = 0; v < nn; ++v) {
        if (f[v] != -1) continue;
        // the leaves reachable through splits end disjoint subtrees: at most 2^depth of them
        if (cnt >= (1 << depth)) break;
        ShapLeaf* L = out + cnt;
        const int dep = 31 - __clz(v + 1);
        int m = 0;
        bool ok = true;
        for (int s = dep; s >= 1; --s) {
            const int a = ((v + 1) >> s) - 1, c = ((v + 1) >> (s - 1)) - 1;
            const int k = f[a];
            if (k < 0 || k >= p) {
                ok = false;
                break;
            }
            const double ratio = (double)cv[c] / (double)cv[a];
            int j = 0;
            while (j < m && L->col[j] != k) ++j;
            if (j == m) {                                      // m < dep <= depth <= kMaxD here
                L->col[j] = k;
                L->z[j] = ratio;
                L->mask[j] = 0;
                L->want[j] = 0;
                ++m;
            } else {
                L->z[j] = L->z[j] * ratio;
            }
            L->mask[j] |= 1ull << a;                           // a < 2^depth - 1 <= 63
            if (c == 2 * a + 1) L->want[j] |= 1ull << a;
        }
        if (!ok) continue;
        double b = vl[v];
        if (m > 0) {
            double P = L->z[0];
            for (int j = 1; j < m; ++j) P = P * L->z[j];
            b = vl[v] * P;
        }
        L->val = vl[v];
        L->bias = b;
        L->m = m;
        L->pad = 0;
        for (int j = m; j < kMaxD; ++j) {
            L->col[j] = 0;
            L->z[j] = 0.0;
            L->mask[j] = 0;
            L->want[j] = 0;
        }
        ++cnt;
    }
    nleaf[r] = cnt;
}

__host__ __device__ constexpr double shap_fact(int k) {
    return k <= 1 ? 1.0 : (double)k * shap_fact(k - 1);
}
// W[m][k] = (double)(k! (m-1-k)!) / (double)(m!)
__host__ __device__ constexpr double shap_w(int m, int k) {
    return (shap_fact(k) * shap_fact(m - 1 - k)) / shap_fact(m);
}

// for (I = A; I < B; ++I) f(I) with I a compile-time constant in the body
template <int A, int B, class F>
__device__ __forceinline__ void shap_static_for(F&& f) {
    if constexpr (A < B) {
        f(std::integral_constant<int, A>{});
        shap_static_for<A + 1, B>(f);
    }
}

// The M terms of one leaf into the lane's accumulators acc[col * 64] (the wave's LDS file, this
// lane's slot).  Every index below is a compile-time constant, so c, z and o stay in registers and
// the weights are immediates.
template <int M>
__device__ __forceinline__ void shap_leaf_terms(const ShapLeaf* L, u64 cmp, double* acc) {
    double z[M], o[M];
    shap_static_for<0, M>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        z[j] = L->z[j];
        o[j] = ((cmp ^ L->want[j]) & L->mask[j]) == 0 ? 1.0 : 0.0;
    });
    const double val = L->val;
    shap_static_for<0, M>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        double c[M];
        c[0] = 1.0;
        shap_static_for<0, M>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if constexpr (j != d) {
                constexpr int n = 1 + j - (j > d ? 1 : 0);         // coefficients so far
                c[n] = c[n - 1] * o[j];
                shap_static_for<1, n>([&](auto ic) {               // k = n - 1 down to 1
                    constexpr int k = n - decltype(ic)::value;
                    c[k] = c[k] * z[j] + c[k - 1] * o[j];
                });
                c[0] = c[0] * z[j];
            }
        });
        constexpr double w0 = shap_w(M, 0);
        double s = c[0] * w0;
        shap_static_for<1, M>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            constexpr double wk = shap_w(M, k);
            s = s + c[k] * wk;
        });
        double* slot = acc + L->col[d] * 64;
        *slot = *slot + (val * (o[d] - z[d])) * s;
    });
}

// lane `src`'s value of x in every lane (src wave-uniform)
__device__ __forceinline__ double shap_readlane(double x, int src) {
    const i64 b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double((i64)(((u64)hi << 32) | lo));
}

struct ShapArgs {
    const double* base;
    int64_t col_stride, lda, t0, nt;
    const int32_t* cols;
    int p;
    const double* zs;
    const int32_t* feat;
    const double* thr;
    int depth, n_trees;
    double base_score;
    const u64* bits;
    const ShapLeaf* leaves;
    const int32_t* nleaf;
    double* contrib;     // optional
    double* part;        // optional: [nt][nblk][p+1][2]
    i64* cpart;          // with part: [nt][nblk]
};

// One wave per (date, block of 64 assets), one lane per cell.  The accumulators phi [p][64] are
// the wave's LDS: indexed by a wave-uniform column and the lane, so no two lanes share a bank
// row and nothing is atomic.  Per tree: the cell's comparison bits of every split node (the
// values re-read through L2, z computed where it is read), then per leaf two bit operations per
// path element give o_j.  Dynamic LDS: phi [p][64] doubles, then two chunks of leaf records.
__global__ __launch_bounds__(64) void gbt_shap_kernel(const ShapArgs g) {
    extern __shared__ __attribute__((aligned(16))) double shap_acc[];
    const int lane = threadIdx.x;
    const int64_t nblk = g.lda >> 6;
    const int64_t ti = blockIdx.x / nblk, blk = blockIdx.x % nblk;
    const int64_t t = g.t0 + ti, a = blk * 64 + lane;
    const int p = g.p;
    const bool use = (g.bits[(t >> 6) * g.lda + a] >> (t & 63)) & 1ull;
    const u64 set = __ballot(use);
    double* acc = shap_acc + lane;
    double bias = g.base_score;
    if (set != 0) {
        for (int c = 0; c < p; ++c) acc[c * 64] = 0.0;
        const double* cell = g.base + t * g.lda + a;
        const double2* zs2 = reinterpret_cast<const double2*>(g.zs);
        const int nn = (2 << g.depth) - 1, nint = (1 << g.depth) - 1;
        // The leaf records reach the lanes through LDS, kShapChunk at a time and double-buffered:
        // the wave loads the next chunk with two 16-byte loads a lane while it works on this one
        // (a record read straight from memory costs several dependent round trips a leaf).
        char* rec = reinterpret_cast<char*>(shap_acc + (int64_t)p * 64);
        const int slot_bytes = (int)sizeof(ShapLeaf) << g.depth;           // a tree's records
        const char* lbase = reinterpret_cast<const char*>(g.leaves);
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
        auto fetch = [&](int r, int c0) {          // records [c0, c0 + kShapChunk) of tree r
            const char* src = lbase + (int64_t)r * slot_bytes + c0 * (int)sizeof(ShapLeaf);
            const int lim = slot_bytes - c0 * (int)sizeof(ShapLeaf);       // bytes left in the slot
            const int o0 = lane * 16, o1 = 1024 + lane * 16;
            if (o0 < lim) q0 = *reinterpret_cast<const uint4*>(src + o0);
            if (o1 < kShapChunkBytes && o1 < lim) q1 = *reinterpret_cast<const uint4*>(src + o1);
        };
        auto next = [&](int& r, int& c0, int& nl) {    // the next chunk that holds a leaf
            c0 += kShapChunk;
            while (r < g.n_trees && c0 >= nl) {
                ++r;
                c0 = 0;
                nl = r < g.n_trees ? g.nleaf[r] : 0;
            }
        };
        int r = 0, c0 = -kShapChunk, nl = g.n_trees > 0 ? g.nleaf[0] : 0, buf = 0;
        next(r, c0, nl);                               // c0 = 0 of the first tree with a leaf
        if (r < g.n_trees) fetch(r, c0);
        u64 cmp = 0;
        while (r < g.n_trees) {
            char* cur = rec + buf * kShapChunkBytes;
            *reinterpret_cast<uint4*>(cur + lane * 16) = q0;
            if (lane * 16 + 1024 < kShapChunkBytes)
                *reinterpret_cast<uint4*>(cur + 1024 + lane * 16) = q1;
            int r2 = r, c2 = c0, nl2 = nl;
            next(r2, c2, nl2);
            if (r2 < g.n_trees) fetch(r2, c2);
            if (c0 == 0) {                             // a new tree: the cell's comparison bits
                // Lane v reads node v (column, plane, threshold) and the wave takes them by
                // readlane, eight nodes at a time with every load of the eight issued before the
                // first compare.  A node that does not split reads column 0 against -inf: no bit.
                const int32_t* f = g.feat + (int64_t)r * nn;
                const double* th = g.thr + (int64_t)r * nn;
                int kv = 0;
                double tv = -__builtin_inf();
                if (lane < nint) {
                    const int k = f[lane];
                    if (k >= 0 && k < p) {
                        kv = k;
                        tv = th[lane];
                    }
                }
                const int pv = g.cols[kv];
                const u64 splits = __ballot(lane < nint && tv > -__builtin_inf());
                cmp = 0;
                for (int v0 = 0; v0 < nint; v0 += 8) {                     // v0 + 7 <= 63
                    if (((splits >> v0) & 0xffull) == 0) continue;
                    double x[8];
                    double2 ms[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int k = __builtin_amdgcn_readlane(kv, v0 + i);
                        const int plane = __builtin_amdgcn_readlane(pv, v0 + i);
                        x[i] = cell[(int64_t)plane * g.col_stride];
                        if (zs2) ms[i] = zs2[(int64_t)k * g.lda + a];
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const double tt = shap_readlane(tv, v0 + i);
                        const double xx = zs2 ? (x[i] - ms[i].x) * ms[i].y : x[i];
                        cmp |= xx < tt ? 1ull << (v0 + i) : 0ull;
                    }
                }
            }
            __syncthreads();                           // one wave: the chunk is in LDS
            const int cnt = min(kShapChunk, nl - c0);
            const ShapLeaf* L = reinterpret_cast<const ShapLeaf*>(cur);
            for (int l = 0; l < cnt; ++l, ++L) {
                bias = bias + L->bias;
                switch (__builtin_amdgcn_readfirstlane(L->m)) {
                    case 1: shap_leaf_terms<1>(L, cmp, acc); break;
                    case 2: shap_leaf_terms<2>(L, cmp, acc); break;
                    case 3: shap_leaf_terms<3>(L, cmp, acc); break;
                    case 4: shap_leaf_terms<4>(L, cmp, acc); break;
                    case 5: shap_leaf_terms<5>(L, cmp, acc); break;
                    case 6: shap_leaf_terms<6>(L, cmp, acc); break;
                    default: break;                    // a root leaf: the bias only
                }
            }
            r = r2;
            c0 = c2;
            nl = nl2;
            buf ^= 1;
        }
    }
    const double nan = __builtin_nan("");
    for (int c = 0; c <= p; ++c) {
        const double v = set == 0 ? 0.0 : (c == p ? bias : acc[c * 64]);
        if (g.contrib) g.contrib[(ti * (p + 1) + c) * g.lda + a] = use ? v : nan;
        if (g.part) {
            double s = use ? v : 0.0, sa = fabs(s);
            for (int st = 32; st > 0; st >>= 1) {          // lanes i < st hold s[i] + s[i + st]
                s = s + __shfl_down(s, st);
                sa = sa + __shfl_down(sa, st);
            }
            if (lane == 0) {
                double* out = g.part + ((ti * nblk + blk) * (p + 1) + c) * 2;
                out[0] = s;
                out[1] = sa;
            }
        }
    }
    if (g.part && lane == 0) g.cpart[ti * nblk + blk] = (i64)__popcll(set);
}

// agg[ti][c][k] = the blocks' partial sums in ascending order; cnt[ti] likewise (integers).
__global__ __launch_bounds__(256) void gbt_shap_agg_kernel(const double* part, const i64* cpart,
                                                           int64_t nt, int64_t nblk, int p,
                                                           double* agg, i64* cnt) {
    const int64_t per = (int64_t)(p + 1) * 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt * (per + 1)) return;
    const int64_t ti = i / (per + 1), e = i % (per + 1);
    if (e == per) {
        i64 s = 0;
        for (int64_t b = 0; b < nblk; ++b) s += cpart[ti * nblk + b];
        cnt[ti] = s;
        return;
    }
    const double* src = part + ti * nblk * per + e;
    double s = src[0];
    for (int64_t b = 1; b < nblk; ++b) s = s + src[b * per];
    agg[ti * per + e] = s;
}

const char* shap_shape_error(int p, int D, int n_trees) {
    if (p < 1 || p > AFM_GBT_MAX_COLS) return "need 1 <= p <= 256";
    if (D < 1 || D > AFM_GBT_MAX_DEPTH) return "need 1 <= max_depth <= 6";
    if (n_trees < 0 || n_trees > AFM_GBT_SHAP_MAX_TREES) return "need 0 <= n_trees <= 2^20";
    return nullptr;
}

inline bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

}  // namespace

extern "C" int afm_gbt_cover_i64(afm_ctx* ctx, const uint8_t* bins, int64_t n, int64_t n_pad, int p,
                                 const int32_t* w, const int32_t* feat, const int32_t* bin,
                                 int max_depth, int n_trees, int64_t* cover) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(bins && w && feat && bin && cover, "null buffer");
    AFM_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "need 1 <= n < 2^31");
    if (const char* msg = shap_shape_error(p, max_depth, n_trees)) AFM_CHECK_ARG(false, msg);
    AFM_CHECK_ARG(n_pad >= n && n_pad % 64 == 0, "n_pad: a multiple of 64 >= n");
    AFM_CHECK_ARG(aligned16(bins) && aligned16(w), "bins and w must be 16-byte aligned");
    if (n_trees == 0) return AFM_OK;
    const int nn = (2 << max_depth) - 1;
    AFM_HIP(hipMemsetAsync(cover, 0, (size_t)n_trees * nn * 8, ctx->stream));
    const int nslabs = (n_trees + kCovTrees - 1) / kCovTrees;              // <= 32,768
    int64_t rows = ctx->gbt_rows_per_wg;
    if (rows <= 0) {        // about 12 workgroups per CU (3 are resident), chunks of >= 1,024 rows
        const int64_t target = std::max<int64_t>(1, (12 * (int64_t)afm_ctx_cus(ctx)) / nslabs);
        rows = std::max<int64_t>(1024, (n + target - 1) / target);
    }
    rows = std::min<int64_t>(rows, kCovMaxChunk);
    const int64_t nchunks = (n + rows - 1) / rows;                         // < 2^31
    hipLaunchKernelGGL(gbt_cover_kernel, dim3((unsigned)nchunks, (unsigned)nslabs), dim3(256), 0,
                       ctx->stream, bins, n, n_pad, p, w, feat, bin, max_depth, n_trees, rows,
                       reinterpret_cast<u64*>(cover));
    AFM_HIP(hipGetLastError());
    return AFM_OK;
}

extern "C" int64_t afm_gbt_shap_scratch_bytes(int64_t lda, int64_t nt, int p, int max_depth,
                                              int n_trees) {
    const char* msg = shap_shape_error(p, max_depth, n_trees);
    if (!msg && (lda < 64 || lda % 64 != 0)) msg = "lda: a positive multiple of 64";
    if (!msg && (nt < 0 || nt * (lda / 64) >= ((int64_t)1 << 31))) msg = "need 0 <= nt * (lda / 64) < 2^31";
    if (msg) {
        afm_set_error(std::string("afm_gbt_shap_scratch_bytes: ") + msg);
        return AFM_E_ARG;
    }
    return shap_layout(lda, nt, p, max_depth, n_trees).total;
}

extern "C" int afm_gbt_shap_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t lda,
                                int64_t t0, int64_t nt, const int32_t* cols, int p,
                                const double* zs, const int32_t* feat, const double* thr,
                                const double* val, const int64_t* cover, int max_depth,
                                int n_trees, double base_score, const uint64_t* bits,
                                uint64_t* scratch, double* contrib, double* agg, int64_t* cnt) {
    AFM_CTX(ctx);
    AFM_CHECK_ARG(base && cols && feat && thr && val && cover && bits && scratch, "null buffer");
    AFM_CHECK_ARG(contrib || agg, "at least one of contrib and agg");
    AFM_CHECK_ARG((agg == nullptr) == (cnt == nullptr), "cnt goes with agg");
    AFM_CHECK_ARG(lda >= 64 && lda % 64 == 0 && nt >= 0 && t0 >= 0, "bad shape");
    if (const char* msg = shap_shape_error(p, max_depth, n_trees)) AFM_CHECK_ARG(false, msg);
    const int64_t nblk = lda / 64;
    AFM_CHECK_ARG(nt * nblk < ((int64_t)1 << 31), "need nt * (lda / 64) < 2^31");
    AFM_CHECK_ARG(aligned16(scratch), "scratch must be 16-byte aligned");
    if (nt == 0) return AFM_OK;
    const ShapScratch S = shap_layout(lda, nt, p, max_depth, n_trees);
    char* sb = reinterpret_cast<char*>(scratch);
    ShapLeaf* leaves = reinterpret_cast<ShapLeaf*>(sb + S.leaves);
    int32_t* nleaf = reinterpret_cast<int32_t*>(sb + S.nleaf);
    double* part = reinterpret_cast<double*>(sb + S.part);
    i64* cpart = reinterpret_cast<i64*>(sb + S.cpart);
    hipStream_t st = ctx->stream;
    if (n_trees > 0) {
        hipLaunchKernelGGL(gbt_shap_path_kernel, dim3((unsigned)((n_trees + 63) / 64)), dim3(64), 0,
                           st, feat, val, reinterpret_cast<const i64*>(cover), p, max_depth,
                           n_trees, leaves, nleaf);
        AFM_HIP(hipGetLastError());
    }
    ShapArgs g;
    g.base = base;
    g.col_stride = col_stride;
    g.lda = lda;
    g.t0 = t0;
    g.nt = nt;
    g.cols = cols;
    g.p = p;
    g.zs = zs;
    g.feat = feat;
    g.thr = thr;
    g.depth = max_depth;
    g.n_trees = n_trees;
    g.base_score = base_score;
    g.bits = reinterpret_cast<const u64*>(bits);
    g.leaves = leaves;
    g.nleaf = nleaf;
    g.contrib = contrib;
    g.part = agg ? part : nullptr;
    g.cpart = cpart;
    // the accumulators and two chunks of leaf records: 52,736 B at p = 97, 134,144 B at p = 256
    const int lds = p * 64 * (int)sizeof(double) + 2 * kShapChunkBytes;
    AFM_HIP(afm_lds_opt_in(ctx, reinterpret_cast<const void*>(gbt_shap_kernel), lds));
    hipLaunchKernelGGL(gbt_shap_kernel, dim3((unsigned)(nt * nblk)), dim3(64), (size_t)lds, st, g);
    AFM_HIP(hipGetLastError());
    if (agg) {
        const int64_t items = nt * ((int64_t)(p + 1) * 2 + 1);
        hipLaunchKernelGGL(gbt_shap_agg_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0,
                           st, part, cpart, nt, nblk, p, agg, reinterpret_cast<i64*>(cnt));
        AFM_HIP(hipGetLastError());
    }
    return AFM_OK;
}
