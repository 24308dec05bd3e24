/* afm_gbt_shap.h -- what the boosted trees of afm_gbt.h are made of: the cover of every node (the
 * sum of the weights of the rows that reach it) and the exact path-dependent TreeSHAP contributions
 * of every column to every prediction (XGBoost's pred_contribs), per cell and per date.
 * Conventions as in afm.h and afm_gbt.h (device buffers, status returns, afm_last_error()).
 *
 * Trees are afm_gbt.h's arrays feat / bin / thr / val [n_trees][nn] in heap order, nn =
 * 2^(max_depth+1) - 1 (the children of node v are 2v+1 and 2v+2; feat >= 0: the split column, -1:
 * a leaf, -2: absent).  New beside them: cover, int64 [n_trees][nn].
 *
 * Cover.  cover[r][v] = the sum of w_i over the rows i < n that reach node v of tree r: every row
 * starts at the root and at a split moves right iff bins[feat[v]][i] > bin[v] (the fit's routing),
 * else left.  Nodes no row reaches, absent ones among them, get 0.  Integer adds only: the same
 * bits whatever the work split (the context option "gbt_rows_per_wg").  For the rows and weights
 * of a fit it is the H of afm_gbt.h.
 *
 * Contributions.  The algorithm is fixed to the last bit (tests/gbt_shap_ref.py restates it in
 * numpy): every operator below is one IEEE fp64 operation, no FMA contraction.  For one cell with
 * values x (column k: plane cols[k] at the cell, z-scored by zs row k when zs is given), phi[0..p)
 * and the bias start from +0.0 and base_score.  The trees r = 0..n_trees-1 are taken in order, in
 * a tree the leaves (feat == -1) in heap order.  For a leaf l:
 *
 *   The path from the root to l is a list of splits (v, child).  Its splits are merged by column:
 *   the m <= max_depth distinct columns d_0..d_{m-1}, in the order of first appearance from the
 *   root.  For element j:
 *     z_j = the product, root to leaf, over the path's splits on d_j of
 *           (double)cover[child] / (double)cover[v]   (one division each; the first ratio starts
 *           the product);
 *     o_j = 1.0 if the cell agrees with the path at every one of those splits, else 0.0 -- a cell
 *           goes left iff x < thr[v], afm_gbt_predict_f64's rule.
 *   For every element d, c = the coefficients in t of the product over j != d of (z_j + o_j t):
 *   c starts as [1.0]; the factors j are multiplied in in path order; with n coefficients
 *   c[0..n), a factor gives c'[n] = c[n-1] * o_j, c'[k] = c[k] * z_j + c[k-1] * o_j for
 *   0 < k < n, and c'[0] = c[0] * z_j.
 *     W[m][k] = (double)(k! (m-1-k)!) / (double)(m!);
 *     s_d = c[0] * W[m][0], then s_d = s_d + c[k] * W[m][k] for k = 1..m-1;
 *     phi[d_d] = phi[d_d] + (val[l] * (o_d - z_d)) * s_d.
 *   bias = bias + val[l] * (z_0 * z_1 * ... * z_{m-1}), the product left to right; a root leaf
 *   (m = 0) adds val[0].
 *
 * A column no tree splits on keeps +0.0.  The sum of phi and the bias is the prediction up to
 * rounding.  A present node with cover 0, a tree whose leaves are not all reachable through
 * splits, or a cover that is not the sum of its children's is the caller's error: the result is
 * then unspecified (NaN or inf may appear), and nothing faults.
 */
#ifndef AFM_GBT_SHAP_H
#define AFM_GBT_SHAP_H

#include "afm_gbt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_GBT_SHAP_MAX_TREES 1048576

/* Argument rules (AFM_E_ARG, nothing is launched): afm_gbt.h's common rules (p, max_depth, n,
 * n_pad, null buffers that are not marked optional, 16-byte alignment of bins, w and scratch), and
 * n_trees outside 0..AFM_GBT_SHAP_MAX_TREES. */

/* cover [n_trees][nn] as defined above (overwritten; w <= 0 counts as 0, w <= AFM_GBT_MAX_WEIGHT).
 * A workgroup owns a chunk of rows and a slab of 32 trees and counts each row in LDS at the node
 * where it settles (32-bit integer adds); a split's count is the sum of its children's; the slabs
 * are merged with 64-bit integer atomics. */
int afm_gbt_cover_i64(afm_ctx* ctx, const uint8_t* bins, int64_t n, int64_t n_pad, int p,
                      const int32_t* w, const int32_t* feat, const int32_t* bin, int max_depth,
                      int n_trees, int64_t* cover);

/* Bytes of afm_gbt_shap_f64's scratch (the flattened paths and the per-block partial sums of the
 * aggregates).  Negative (afm_last_error() set) on lda not a positive multiple of 64, nt < 0, or
 * bad p, max_depth or n_trees. */
int64_t afm_gbt_shap_scratch_bytes(int64_t lda, int64_t nt, int p, int max_depth, int n_trees);

/* The contributions of the first n_trees trees on the grid rows with a bit set, t in [t0, t0+nt):
 * afm_gbt_predict_f64's addressing, zs (optional) and bits.
 *   contrib (optional) [nt][p+1][lda], date t at index t - t0, the asset fastest, column p the
 *     bias; NaN on the cells of those dates whose bit is not set.
 *   agg (optional) [nt][p+1][2] = {sum phi, sum |phi|} over the date's set cells, in a pinned
 *     order: in a block of 64 consecutive assets the tree s[i] = s[i] + s[i+st], st = 32, 16, ..
 *     1, with +0.0 for a cell that is not set; then the blocks' sums s_0 + s_1 + ..., ascending.
 *     The result does not depend on the grid or on how a date range is cut into calls.
 *   cnt (with agg, else NULL) int64 [nt]: the date's set cells.
 * At least one of contrib and agg is given.  n_trees = 0: phi = +0.0 and bias = base_score.
 * Also AFM_E_ARG: lda not a multiple of 64 or < 64, nt or t0 negative, nt * (lda / 64) >= 2^31. */
int afm_gbt_shap_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t lda,
                     int64_t t0, int64_t nt, const int32_t* cols, int p, const double* zs,
                     const int32_t* feat, const double* thr, const double* val,
                     const int64_t* cover, int max_depth, int n_trees, double base_score,
                     const uint64_t* bits, uint64_t* scratch, double* contrib, double* agg,
                     int64_t* cnt);

#ifdef __cplusplus
}
#endif

#endif /* AFM_GBT_SHAP_H */
