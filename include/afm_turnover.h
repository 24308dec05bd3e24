/* afm_turnover.h -- the stability half of the factor screen on the MI355X engine: how much a
 * column changes from one evaluated date to an earlier one.  Per (date, column, lag) the rank
 * autocorrelation, the turnover of the extreme decile layers and the turnover of the
 * factor-weighted top-10 book, and their means over the dates.  Conventions as in afm.h (device
 * buffers, calendar grids, status returns, afm_last_error()).
 *
 * In pandas: groupby('date').rank() pivoted and correlated with its own shift(lag), and set
 * differences of the layer / top-10 members of two dates.
 */
#ifndef AFM_TURNOVER_H
#define AFM_TURNOVER_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_TURNOVER_MAX_LAGS 8

/* Bytes of the scratch afm_screen_turnover_f64 needs for nd evaluated dates of K columns on planes
 * of lda assets (whatever the lags are).  Negative (afm_last_error() set): lda is not a positive
 * multiple of 64 up to 32768, nd < 0 or K < 1. */
int64_t afm_screen_turnover_scratch_bytes(int64_t nd, int K, int64_t lda);

/* The arguments up to nrows are afm_xs_preprocess_f64's: dates DEVICE int32 [nd] (the evaluated
 * dates, paired by position), the value v(t, a) of asset a = rows_idx[t][e], e < nrows[t], is the
 * double the IC kernel reads -- plane base + cols[k] * col_stride at [t][a], with zs z = (x - mu) *
 * (1/sd) of row zcols[k] (NULL = row k).  A NaN value has no rank; +-inf is ranked and -0.0 ties
 * with 0.0 (afm_screen_layers_f64's rule).  lags: HOST int32 [L], every lag >= 1, in any order,
 * repeats allowed.
 *
 * For position i, column k and lag = lags[l], t1 = dates[i] and t0 = dates[i - lag]:
 *   rank_ac [nd][K][L]    rho(t, a) = the doubled average-tie ascending rank of v(t, a) among the
 *                         ranked rows of t; over the n assets ranked on both dates, x = rho(t0, .),
 *                         y = rho(t1, .), in int64 cxy = n Sxy - Sx Sy, cxx = n Sxx - Sx Sx, cyy =
 *                         n Syy - Sy Sy (exact), and (double)cxy / sqrt((double)cxx * (double)cyy),
 *                         one IEEE rounding per conversion and operation; NaN when n < 2 or the
 *                         root is 0.
 *   counts [nd][K][L][5]  int32 {n, n_top, new_top, n_bot, new_bot}: top(t) / bot(t) = the rows of
 *                         layer 10 / layer 1 of afm_screen_layers_f64 (int(rank_first / n_k * 10) +
 *                         1, at most 10, ties by row position); n_top = |top(t1)|, new_top =
 *                         |top(t1) \ top(t0)|, and the same for bot.
 *   port_turn [nd][K][L]  P(t) = the ranked rows of descending method='first' rank <= 10, S(t) =
 *                         the sum of their values from 0.0 in rank order, w = f / S(t); 0.5 * the
 *                         sum over P(t0) u P(t1) in ascending asset index of |w(t1, a) - w(t0, a)|
 *                         (a missing side is 0.0), one add per term from 0.0; NaN when a date has
 *                         no ranked row or a weight is not finite.
 * For i < lag: NaN, five zeros, NaN.  Only rows [0, nd) are written.  An item is a function of its
 * two dates' rows and values alone: the same bits whatever K, its place in cols, the other lags
 * and the other dates are.
 *
 * scratch: afm_screen_turnover_scratch_bytes(nd, K, lda) bytes.
 * AFM_E_ARG (nothing is launched): K < 1; lda not a positive multiple of 64 up to 32768; L outside
 * 1..AFM_TURNOVER_MAX_LAGS; a lag < 1; nd < 0 or nd * K * L >= 2^31; a null buffer.  nd == 0
 * returns AFM_OK at once. */
int afm_screen_turnover_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                            int64_t lda, const int32_t* cols, int K, const double* zs,
                            const int32_t* zcols, const int32_t* dates, int64_t nd,
                            const int32_t* rows_idx, const int32_t* nrows, const int32_t* lags,
                            int L, double* rank_ac, int32_t* counts, double* port_turn,
                            uint64_t* scratch);

/* stats [K][L][4][2] = {n, mean} of the four series rank_ac, new_top / n_top, new_bot / n_bot (a
 * date with an empty layer has none) and port_turn over their non-NaN dates, summed in ascending
 * position from 0.0, one add per date; mean NaN when n is 0.  nd == 0 gives {0, NaN}. */
int afm_screen_turnover_summary_f64(afm_ctx* ctx, const double* rank_ac, const int32_t* counts,
                                    const double* port_turn, int64_t nd, int K, int L,
                                    double* stats);

#ifdef __cplusplus
}
#endif

#endif /* AFM_TURNOVER_H */
