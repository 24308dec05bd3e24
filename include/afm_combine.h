/* afm_combine.h -- factor combination on the MI355X engine: the step after the factor screen.  On
 * every evaluated date the screened columns are weighted by what their recent ICs say -- the
 * rolling mean IC, the rolling ICIR, or the rolling "max-IR" weights inv(Sigma) * mean IC with a
 * shrunk IC covariance, all taken strictly from the past -- and combined into one [T][lda] plane,
 * composite[t][a] = sum_k w[t][k] x_k[t][a].  Conventions as in afm.h (device buffers, calendar
 * grids, status returns, afm_last_error()).
 *
 * In pandas: a rolling() over the IC frame, a solve per date, and a groupby('date') multiply-add
 * over K columns.
 */
#ifndef AFM_COMBINE_H
#define AFM_COMBINE_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_COMBINE_EQUAL 0
#define AFM_COMBINE_IC 1
#define AFM_COMBINE_ICIR 2
#define AFM_COMBINE_MAXIR 3
#define AFM_COMBINE_MAX_K 128
#define AFM_COMBINE_MAX_WINDOW 1024

/* w [nd][K] and info [nd][3] = {n_active, n_dates, sum |raw|} from ic [nd][K][3] as
 * afm_screen_ic_f64 wrote it; the positions 0..nd-1 are the evaluated dates in ascending time and
 * q in 0..2 is the return type.  For position i the window is J = {j : max(0, i - embargo -
 * window + 1) <= j <= i - embargo}, empty where i < embargo.  F_k = the j of J with ic[j][k][q]
 * finite, n_k = |F_k|.
 *   AFM_COMBINE_EQUAL: raw_k = 1 for every column on every position; no window is read,
 *     n_dates = 0.
 *   AFM_COMBINE_IC: column k is active when n_k >= min_periods; raw_k = m_k = (sum of ic over
 *     F_k) / n_k; n_dates = max_k n_k.
 *   AFM_COMBINE_ICIR: s_k = sqrt(sum (ic - m_k)^2 / (n_k - 1)); active when additionally s_k is
 *     finite and > 0; raw_k = m_k / s_k.
 *   AFM_COMBINE_MAXIR: the columns with n_k >= min_periods are candidates; D = the j of J on
 *     which every candidate's IC is finite, n_dates = |D|; with |D| < min_periods (or no
 *     candidate) no column is active.  m, S (ddof 1): the mean vector and covariance of the
 *     candidates' ICs over D; a candidate with S_kk not > 0 is dropped, D stays.  A = (1 - shrink)
 *     S + shrink diag(S) over the active columns, raw = inv(A) m by Cholesky.
 * w_k = raw_k / sum_active |raw|, 0 for an inactive column.  The whole row of w is NaN when no
 * column is active, when the sum is 0 or not finite, or, for MAXIR, when a pivot is not > 0 (then
 * info[2] is NaN).  info is written for every position.
 *
 * Only ic[j] with j <= i - embargo is read for row i.  Methods 0..2: every sum is taken in
 * ascending j (the window) or ascending k (the normalisation) from 0.0, one add per term, no FMA:
 * a plain numpy loop reproduces them bit for bit.  MAXIR has no stated order but is a function of
 * its own window alone: the same bits whatever nd and whatever lies outside the window.
 *
 * AFM_E_ARG (nothing is written): K outside 1..128; window outside 1..1024; embargo < 0;
 * min_periods outside 1..window, or < 2 for methods 2 and 3; q outside 0..2; an unknown method;
 * shrink outside (0, 1] for method 3; nd < 0; a null buffer.  nd == 0 returns AFM_OK at once. */
int afm_ic_weights_f64(afm_ctx* ctx, const double* ic, int64_t nd, int K, int q, int method,
                       int window, int embargo, int min_periods, double shrink, double* w,
                       double* info);

/* The arguments up to nrows are afm_xs_preprocess_f64's: for evaluated date i (t = dates[i],
 * DEVICE int32 [nd], any order) the value x_k of row e < nrows[t] is the double the IC kernel
 * reads -- plane base + cols[k] * col_stride at [t][rows_idx[t][e]], with zs z = (x - mu) * (1/sd)
 * of row zcols[k] (NULL = row k).  w: DEVICE [nd][K] with w_stride = K, or one row for all dates
 * with w_stride = 0.
 *
 * Column k is present for a row when x_k is finite and w[i][k] is finite and not 0.  num = the sum
 * over the present k, ascending, of w * x (one rounded multiply, then one add per term, from 0.0);
 * den = the sum of |w| over the same k; out[t][rows_idx[t][e]] = num / den, NaN when no column is
 * present; cnt (int32 [T][lda], may be NULL) gets the number of present columns.  The whole [lda]
 * row of an evaluated date is written -- NaN / 0 off the rows -- and the rows of other dates are
 * not touched.  A repeat in cols counts twice.
 *
 * AFM_E_ARG: K outside 1..128; lda % 64 != 0; w_stride other than 0 or K; out overlapping a plane
 * it reads (cols is copied to the host for this check: the call waits for the context's stream).
 * nd == 0 returns AFM_OK at once. */
int afm_combine_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T, int64_t lda,
                    const int32_t* cols, int K, const double* zs, const int32_t* zcols,
                    const int32_t* dates, int64_t nd, const int32_t* rows_idx,
                    const int32_t* nrows, const double* w, int64_t w_stride, double* out,
                    int32_t* cnt);

#ifdef __cplusplus
}
#endif

#endif /* AFM_COMBINE_H */
