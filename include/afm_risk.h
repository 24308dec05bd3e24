/* afm_risk.h -- the multi-factor risk model of the MI355X engine: an EWMA covariance of the factor
 * returns, an EWMA specific variance per security, the covariance B F B' + D of a book, the risk
 * decomposition of the books, and the box-QP weight solve of afm.h / afm_mv.h from a supplied
 * covariance.  Conventions as in afm.h (device buffers, calendar grids [T][lda] with lda a multiple
 * of 64, row-bit words [ceil(T/64)][lda], status returns, afm_last_error()).
 *
 * Everything is fp64.  The arithmetic is fixed to the last bit (tests/risk_ref.py restates it in
 * numpy): every operator below is one IEEE operation, no FMA contraction, and every sum starts from
 * +0.0 and adds its terms in the order given.
 *
 * The model.  The factors are [1, x_1..x_p], K1 = p + 1 <= AFM_RISK_MAX_FACTORS (x_j: plane cols[j-1]
 * of the panel, column c at base + c * col_stride).  The factor return of date t is
 * f_t = beta[t][0..K1), the per-date OLS of the label plane on the exposure planes over a row-bit
 * mask (afm_xs_gram_f64 + afm_ols_solve_f64).  Date t is USED when rank[t] == p (no regressor was
 * dropped) and every coefficient is finite; unused dates update nothing.  lambda =
 * pow(0.5, 1.0 / half_life) (the C library's pow).
 *
 * Factor covariance (West's weighted update), state (W, m[K1], C[K1][K1]) = 0, for each used date in
 * date order:
 *     lw = lambda * W;  Wn = lw + 1.0;  g = lw / Wn;
 *     d_i = f_i - m_i;  m_i = m_i + d_i / Wn;
 *     C[i][j] = lambda * C[i][j] + (g * d_i) * d_j   for i >= j, mirrored to [j][i];
 *     W = Wn.
 * fcov[t] = C / W (one division per element) from the state after the used dates <= t - lag, and
 * nused[t] counts them; fcov[t] is NaN while nused[t] < min_obs.
 *
 * Residuals.  u[t][a] = y - acc, acc = beta[t][0], then acc = acc + beta[t][j] * x_j for j = 1..p.
 * NaN where the row bit is off, where y or any x_j is not finite, where the date is unused, and on
 * the pad columns a >= A.
 *
 * Specific variance, per security over its own finite residuals in date order, state (W, D, n) = 0:
 *     W = lambda_s * W + 1.0;  D = lambda_s * D + u * u;  n = n + 1.
 * spec[t][a] = D / W from the state after the dates <= t - lag; NaN while n < min_obs and on the pad
 * columns.  fill[t] = the mean of the finite spec[t][a], a < A: their sum in ascending a as
 * np.add.reduce forms it (numpy's pairwise sum of each run of 8192 values, the runs added in order)
 * divided by their count; NaN when there is none.
 *
 * Book.  For a rebalance date (grid date t = dates[i]) and a side with members a_0..a_{k-1}
 * (books[i][side][0..k)), weights w and exposures B[m][0] = 1, B[m][j] = x_j at (t, a_m), a
 * non-finite exposure counting as 0, with F = fcov[t]:
 *     G[m][j] = sum_i B[m][i] * F[i][j], i ascending;
 *     S[m][n] = sum_j G[m][j] * B[n][j], j ascending, formed for m >= n only and mirrored;
 *     d_m = spec[t][a_m], or fill[t] when that is not finite (such members are counted);
 *     S[m][m] = S[m][m] + d_m;
 *     x_i = sum_m B[m][i] * w_m, m ascending;   (F x)_i = sum_j F[i][j] * x_j, j ascending;
 *     c_i = x_i * (F x)_i: the contribution of factor i;  factor variance = sum_i c_i, i ascending;
 *     specific variance = sum_m (w_m * w_m) * d_m, m ascending;  total = factor + specific.
 * The net book (side index 2) is h = (w_L - w_S) / 2.0 over the union of both sides: the long
 * members in book order, then the short members that are not in the long book, in book order; a
 * side a name is not in counts as weight 0.0, and a name in both books is one holding.  It has the
 * risk numbers and contributions of a book and no covariance.
 * A date whose fcov[t] has a non-finite entry, or a book one of whose members needs a fill[t] that
 * is NaN, gets status bit 4; the covariance, risk and contribution rows of that book are NaN.
 */
#ifndef AFM_RISK_H
#define AFM_RISK_H

#include "afm_mv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_RISK_MAX_FACTORS 32

/* Argument rules of every entry point (AFM_E_ARG, nothing is launched): a null buffer that is not
 * marked optional; p outside 1..AFM_RISK_MAX_FACTORS - 1; T or A < 1, lda < A or not a multiple of
 * 64; half_life not finite or <= 0; min_obs < 1; lag < 0. */

/* resid [T][lda] as defined above, every cell written.  One wide launch: the p exposure planes and
 * the label plane ycol are read once, the dates are independent. */
int afm_risk_resid_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T, int64_t A,
                       int64_t lda, const int32_t* cols, int p, int ycol, const double* beta,
                       const int32_t* rank, const uint64_t* bits, double* resid);

/* fcov [T][K1][K1] and nused [T] from beta [T][K1] and rank [T].  One workgroup, one lane per pair
 * i >= j, sequential in the dates; the rows of beta are staged through LDS 64 dates at a time. */
int afm_risk_factor_cov_f64(afm_ctx* ctx, const double* beta, const int32_t* rank, int64_t T,
                            int p, double half_life, int min_obs, int lag, double* fcov,
                            int32_t* nused);

/* spec [T][lda] and fill [T] from resid [T][lda] (half_life: the specific half-life).  One lane per
 * security walking its column in date order with its loads several dates ahead, then one workgroup
 * per date for fill. */
int afm_risk_specific_f64(afm_ctx* ctx, const double* resid, int64_t T, int64_t A, int64_t lda,
                          double half_life, int min_obs, int lag, double* spec, double* fill);

/* The books of a rebalance result (k [nd], books and weights [nd][2][AFM_MAX_BOOK] of
 * afm_rebalance_f64) priced by the model at the dates' grid indices `dates` (DEVICE int32 [nd], each
 * in [0, T)).  One workgroup per (date, side) and one for the net book.  Outputs:
 *   cov     [nd][2][kc][kc]: S of the long and the short book, rows and columns past k not written;
 *   risk    [nd][3][4] = {total, factor, specific variance, members whose d_m was filled}, for the
 *           long, short and net book;
 *   contrib [nd][3][K1];
 *   status  [nd] (overwritten): 0, |4 as defined above, |2 for a date whose k exceeds kc (nothing
 *           else is written for it).
 * 1 <= kc <= AFM_MAX_BOOK, and kc must be at least the largest k: the rebalance's top_n. */
int afm_risk_book_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T, int64_t lda,
                      const int32_t* cols, int p, const int32_t* dates, int64_t nd,
                      const int32_t* k, const int32_t* books, const double* weights,
                      const double* fcov, const double* spec, const double* fill, int kc,
                      double* cov, double* risk, double* contrib, int32_t* status);

/* One book from a supplied covariance: minimise 1/2 w'S w - gamma * mu'w subject to sum w = 1,
 * lo <= w <= hi, with S = cov [k][k] (row-major; the lower triangle is read).  mu: DEVICE [k] (a
 * non-finite value counts as 0) or NULL = no return term.  After loading S the kernel runs exactly
 * the branches afm_min_variance_weights_f64 / afm_mean_variance_weights_f64 run after their
 * covariance phase: fed the cov they returned it gives their weights bit for bit.  status [1]: 0, or
 * 1 (iteration cap or a non-finite covariance: weights NaN).  1 <= k <= AFM_MAX_BOOK, gamma finite
 * and >= 0, lo <= hi. */
int afm_cov_weights_f64(afm_ctx* ctx, const double* cov, int k, const double* mu, double gamma,
                        double lo, double hi, double* w, int32_t* status);

/* Every (date, side) of an afm_rebalance_f64 / afm_rebalance_mv_f64 result solved again from
 * cov [nd][2][kc][kc] (afm_risk_book_f64's, or any other).  mu ([T][lda] plane read at the dates, or
 * NULL = no return term) and gamma as in afm_mv.h, sign -1 on the short book.  weights and sums are
 * rewritten, the sums in afm_rebalance_f64's two summation orders; k, books, upos and usize are
 * only read.  kc <= 32 runs afm_rebalance_f64's solver for top_n <= 32, a larger kc the one for
 * larger books: with kc = top_n and the covariance the rebalance itself formed, its weights and sums
 * come back bit for bit.  cov_status [nd] (optional): on a date with bit 4 set the incoming weights
 * and sums are kept and 4 is ORed into status; on every other date bit 1 of status is recomputed by
 * this solve.  A date with status bit 2, with k = 0 or with k > kc is left alone. */
int afm_rebalance_cov_f64(afm_ctx* ctx, int64_t T, int64_t lda, const int32_t* dates, int64_t nd,
                          const int32_t* k, const int32_t* books, const double* cov, int kc,
                          const int32_t* cov_status, const double* mu, double gamma, double lo,
                          double hi, const double* close, const double* tmr, double* weights,
                          double* sums, int32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* AFM_RISK_H */
