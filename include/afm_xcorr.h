/* afm_xcorr.h -- the other half of the factor screen on the MI355X engine: how the screened
 * columns relate to EACH OTHER.  The per-date cross-sectional correlation matrix of K factor
 * columns on the rows afm_screen.h's IC uses, and its summary over the dates -- what a redundancy
 * pruning of the columns (afm.screen.select_factors) is decided on.  Conventions as in afm.h
 * (device buffers, calendar grids, status returns, afm_last_error()).
 *
 * In pandas: df.groupby('date')[columns].corr() of the screened frame (pairwise complete,
 * min_periods = 1), then the mean and the mean absolute value of every pair over the dates.
 */
#ifndef AFM_XCORR_H
#define AFM_XCORR_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xc [nd][K][K]: for evaluated date i (t = dates[i], DEVICE int32 [nd], any order) the
 * DataFrame.corr() of the date's K columns.  The arguments up to nrows are afm_screen_ic_f64's
 * and the value of a row is the same double: plane base + cols[k] * col_stride at
 * [t][rows_idx[t][e]], with zs z = (x - mu) * (1/sd) of row zcols[k] (NULL = row k).  `rows` is
 * kept so that the call has afm_screen_ic_f64's shape; it is NOT read and may be NULL (the
 * factor-to-factor correlation needs no return plane).
 *
 * A cell that is not finite (NaN, +-inf, a z that came out non-finite) is missing for its column;
 * a pair uses the rows where both columns are present; the entry is NaN with fewer than 2 such
 * rows or where either variance over them is 0, else cov / sqrt(var_j var_k) clipped to [-1, 1].
 * The matrix is full and bitwise symmetric.  An entry of a column with itself -- the diagonal, and
 * a pair of positions that name the same column (and zs row) -- is exactly 1.0 where the column
 * has a non-zero variance on the date, else NaN.
 *
 * Moments on fp64 MFMA, not pandas' Welford recurrence: each column is first shifted by its first
 * finite value of the date and by the mean of that, and scaled by 1 / sd over its own finite rows
 * (a column constant over the date becomes exactly 0: NaN row and column); then per pair
 * N = M'M, P = U'U, S = U'M, Q = (U.U)'M over the rows (M the 0/1 presence, U the standardised
 * values, 0 where missing), cov ~ P - S_jk S_kj / N, var_j|k ~ Q_jk - S_jk^2 / N.  An entry is a
 * function of its two columns' values on the date's rows alone: bitwise the same whatever K, the
 * positions in cols, the other columns and dates of the call, and whether the workgroup took the
 * fast path (no missing cell in its columns: only U'U and the column sums are formed).
 * Only the rows [0, nd) of xc are written.  K >= 1, lda % 64 == 0,
 * nd * B (B + 1) / 2 < 2^31 with B = ceil(K / 64). */
int afm_screen_xcorr_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                         int64_t lda, const int32_t* cols, int K, const double* zs,
                         const int32_t* zcols, const int32_t* dates, int64_t nd, const double* rows,
                         const int32_t* rows_idx, const int32_t* nrows, double* xc);
/* stats [K][K][3] = {n, mean r, mean |r|} of every pair over the nd dates in the order given: n
 * the non-NaN entries; the means are the sums of the entries (of their absolute values) with NaN
 * taken as 0 -- numpy's sum of a contiguous 1-D array, np.where(np.isnan(x), 0, x).sum() -- divided
 * by n, NaN where n == 0.  K >= 1, nd >= 0, K * K < 2^31. */
int afm_screen_xcorr_summary_f64(afm_ctx* ctx, const double* xc, int64_t nd, int K, double* stats);

#ifdef __cplusplus
}
#endif

#endif /* AFM_XCORR_H */
