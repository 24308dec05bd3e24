/* afm_gbt.h -- gradient-boosted regression trees on the MI355X engine: the reference's XGBoost
 * models (KKT:481-576, 644-662) on the z-scored panel that is already on the device.  Squared
 * error, histogram splits, level-wise growth.  Conventions as in afm.h (device buffers, calendar
 * grids, status returns, afm_last_error()).
 *
 * The algorithm is fixed to the last bit (tests/gbt_ref.py restates it in numpy): gradients are
 * quantised to integers, so every histogram sum is exact whatever the order of addition, and
 * every floating-point step below is one IEEE fp64 operation (no FMA contraction).
 *
 * Inputs: n rows of p finite doubles, a finite label y and an integer weight w per row, 0 <= w <=
 * AFM_GBT_MAX_WEIGHT: 0 = the row is only evaluated, 1 = it trains, 2 = it enters twice (the rows
 * of train_end in the reference's train+valid fit).  At least one row has w > 0.
 *
 * Cuts of column k: s = the values of the rows with w > 0 sorted ascending, m their count; the
 * candidates s[(j * m) / B], j = 1..B-1 (integer division); cuts[k][0..ncuts[k]) = the distinct
 * candidates ascending, -0.0 stored as 0.0; ncuts[k] <= B - 1 and may be 0.  bin(x) = the number
 * of cuts <= x, 0..ncuts[k].  The bin matrix is uint8 [p][n_pad], one plane per column, n_pad a
 * multiple of 64 >= n.
 *
 * A round: g_i = F_i - y_i; gmax = max |g_i| over w > 0; W = sum w; e = 62 - bit_length(W) - E
 * with gmax = f * 2^E, 0.5 <= f < 1 (frexp), at most 960, and 0 when gmax == 0; q_i = w_i *
 * (int64) rint(g_i * 2^e) (half to even; 0 without the conversion where w_i = 0).  Every sum of q
 * stays below 2^62.
 *
 * The tree grows level by level in heap order (the children of node v are 2v+1 and 2v+2).  A node
 * has G = sum q and H = sum w over its rows (exact) and the value eta * (-((double)G * 2^-e) /
 * ((double)H + lambda)).  Below depth max_depth every (k, b), b < ncuts[k], is a candidate "bin <=
 * b goes left": with GL, HL the left sums, gl = (double)GL * 2^-e, gr = (double)(G - GL) * 2^-e,
 * g = (double)G * 2^-e, it is admissible when HL >= min_child_weight and HR >= min_child_weight,
 * and gain = gl*gl/(HL+lambda) + gr*gr/(HR+lambda) - g*g/(H+lambda), left to right.  The node
 * splits on the admissible candidate of largest gain if that gain is > gamma (ties: lowest k,
 * then lowest b); else it is a leaf.
 *
 * A tree is four arrays of 2^(max_depth+1) - 1 nodes: feat int32 (>= 0: the split column, -1: a
 * leaf, -2: absent), bin int32 (the split's b; -1 on a node that does not split), thr double =
 * cuts[k][b] (0.0 on a node that does not split), val double (the value of every present node,
 * 0.0 on an absent one).  After the tree F_i += val[leaf of i] on every row, w = 0 included.
 * On raw values a row goes left iff x < thr -- the partition of the bins.
 */
#ifndef AFM_GBT_H
#define AFM_GBT_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_GBT_MAX_DEPTH 6
#define AFM_GBT_MAX_BIN 256
#define AFM_GBT_MAX_COLS 256
#define AFM_GBT_MAX_WEIGHT 4095

/* Common argument rules (AFM_E_ARG, nothing is launched): p outside 1..AFM_GBT_MAX_COLS;
 * max_depth outside 1..AFM_GBT_MAX_DEPTH; max_bin outside 2..AFM_GBT_MAX_BIN; n < 1 or n >= 2^31;
 * n_pad not a multiple of 64 or < n; a null buffer that is not marked optional; bins, node, q, w
 * and scratch not 16-byte aligned. */

/* Bytes of afm_gbt_fit_f64's scratch.  Negative (afm_last_error() set) on bad n, p, max_depth or
 * max_bin. */
int64_t afm_gbt_scratch_bytes(int64_t n, int p, int max_depth, int max_bin);

/* out[i] = the value of row i in column k, i < n: the cell (rows_t[i], rows_a[i]) of the plane base
 * + cols[k] * col_stride ([T][lda]); with zs (rows [.][lda][2] = {mu, 1/sd}) z = (x - mu) * (1/sd)
 * of zs row k, zs = NULL: the raw value.  rows_t = NULL: date 0; rows_a = NULL: asset i -- a dense
 * column-major matrix is T = 1, lda = n_pad, both NULL.  The row lists are not validated. */
int afm_gbt_values_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                       int64_t lda, const int32_t* cols, int k, const double* zs,
                       const int32_t* rows_t, const int32_t* rows_a, int64_t n, double* out);

/* bins[k][i] = bin of the value of row i in column k (afm_gbt_values_f64's addressing, every k <
 * p) among cuts [p][max_bin - 1] / ncuts [p]; the rows [n, n_pad) get 0.  Sixteen bins per
 * 16-byte store. */
int afm_gbt_bin_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T, int64_t lda,
                    const int32_t* cols, int p, const double* zs, const int32_t* rows_t,
                    const int32_t* rows_a, int64_t n, int64_t n_pad, const double* cuts,
                    const int32_t* ncuts, int max_bin, uint8_t* bins);

/* One level's histograms hist [nnodes][p][max_bin][2] = {sum q, sum w} (int64) over the rows i < n
 * with 0 <= node[i] < nnodes (any other node value: the row is in none), 1 <= nnodes <= 32.  A
 * workgroup owns a tile of columns and a chunk of rows and accumulates in LDS with integer adds
 * (64-bit for q, 32-bit for w); the workgroups' slabs are merged with integer adds: the same bits
 * whatever the work split (the context option "gbt_rows_per_wg").  A bin byte >= max_bin is not
 * counted. */
int afm_gbt_hist_i64(afm_ctx* ctx, const uint8_t* bins, int64_t n, int64_t n_pad, int p,
                     int max_bin, const int32_t* node, const int64_t* q, const int32_t* w,
                     int nnodes, int64_t* hist);

/* n_rounds rounds on the bin matrix, enqueued without a host synchronisation: the scale exponent
 * is computed and read on the device.  F [n]: in = the start (base_score), out = the fit's value
 * on every row.  Trees feat, bin [n_rounds][2^(max_depth+1) - 1] int32, thr, val likewise double.
 * evals [n_rounds][2][6] = after each round, for the rows with w > 0 and with w = 0, {count, sum F,
 * sum y, sum F^2, sum y^2, sum F y}, each row once, summed in fp64 over a fixed partition and
 * tree: two runs agree bitwise.  scratch: afm_gbt_scratch_bytes(n, p, max_depth, max_bin) bytes.
 * Also AFM_E_ARG: n_rounds < 1, min_child_weight < 1, reg_lambda or gamma negative (or NaN). */
int afm_gbt_fit_f64(afm_ctx* ctx, const uint8_t* bins, int64_t n, int64_t n_pad, int p,
                    const double* cuts, const int32_t* ncuts, const double* y, const int32_t* w,
                    int n_rounds, int max_depth, int max_bin, double eta, double reg_lambda,
                    double gamma, double min_child_weight, int32_t* feat, int32_t* bin,
                    double* thr, double* val, double* F, double* evals, uint64_t* scratch);

/* pred[t][a] = base_score plus one add per tree, the first n_trees trees in order, each walked
 * from the root over the cell's values x_k = plane cols[k] at [t][a], z-scored by zs row k when zs
 * is given (optional); grid rows with a bit set, t in [t0, t0+nt); NaN on the other cells of those
 * dates.  afm_zpredict_f64's arguments with the trees in place of beta.  n_trees >= 0. */
int afm_gbt_predict_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t lda,
                        int64_t t0, int64_t nt, const int32_t* cols, int p, const double* zs,
                        const int32_t* feat, const double* thr, const double* val, int max_depth,
                        int n_trees, double base_score, const uint64_t* bits, double* pred);

#ifdef __cplusplus
}
#endif

#endif /* AFM_GBT_H */
