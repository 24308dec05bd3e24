/* afm_screen_layers.h -- the backtest half of the factor screen on the MI355X engine: the decile
 * layered returns, the long-short spreads and the factor-weighted top-10 return of K factor
 * columns in one pass over the panel, on the row set, forward returns and demeans that
 * afm_screen.h's IC uses.  Conventions as in afm.h (device buffers, calendar grids, status
 * returns, afm_last_error()).
 *
 * The reference gets these one column at a time from AlphaSignalAnalyzer(df_train_x[[c]], c,
 * df_train[['close_price']]).run() (KKT:465, 472): _calc_layered_ret (KKT:324-340) and
 * _backtest_top_stocks (KKT:356-375).  Per column that is afm_xs_layers_f64 + afm_xs_stats_f64 +
 * afm_xs_series_f64 of afm.h; these two entry points do it for every column on the shared
 * preparation (afm_fwd_returns_f64, afm_xs_prepare_f64 with a signal plane that marks the rows).
 * The IC, the IR and the summary stay afm_screen.h's and afm_rankic.h's.
 */
#ifndef AFM_SCREEN_LAYERS_H
#define AFM_SCREEN_LAYERS_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For evaluated date i (t = dates[i], DEVICE int32 [nd], any order) and column k: the values of
 * the column at the date's compacted rows -- the arguments up to nrows are afm_screen_ic_f64's
 * and the value of a row is the same double: plane base + cols[k] * col_stride at
 * [t][rows_idx[t][e]], with zs z = (x - mu) * (1/sd) of row zcols[k] (NULL = row k).  A NaN value
 * has no rank (pandas rank()) and its row is left out for this column; +-inf is ranked like any
 * value, -0.0 ties with 0.0 (this differs on purpose from the IC, which skips what is not
 * finite).  With n_k the rows left, in row order:
 *   layer = int(rank_first / n_k * 10) + 1, at most 10 (KKT:328-330; method='first': ties by row
 *           position; the division in fp64);
 *   layer_cnt [nd][K][10]      the rows of each layer;
 *   layer_mean [nd][K][3][10]  groupby(['date', 'layer']).mean() of each demeaned return over the
 *                              layer's rows in row order (KKT:331; pandas' Kahan group mean), NaN
 *                              for a layer without rows;
 *   port [nd][K][3]            the factor-weighted top-10 return (KKT:359-369): the rows of
 *                              descending method='first' rank <= 10, weights f / sum(f), the
 *                              pivot's string-ordered columns ('1.0', '10.0', '2.0', ...) and
 *                              pandas' NaN-skipping row sums.  The pivot of column k has the ranks
 *                              present on any of its evaluated dates, min(10, max_i n_k(i)) of
 *                              them (found on the device).
 * A (date, column) with n_k == 0: layer_cnt 0, layer_mean NaN, port NaN.  The returns are those
 * of the shared preparation (rows planes 1..3), demeaned over the shared row set and not again per
 * column; a column without NaN on the rows gives what afm_xs_layers_f64 + afm_xs_stats_f64 give
 * for it alone, bit for bit.  Only the rows [0, nd) of the outputs are written.
 * scratch: nd * K * 40 + K doubles (the top-10 cells of every item, the columns' row maxima).
 * K >= 1, lda % 64 == 0, lda <= 32768, nd * K < 2^31. */
int afm_screen_layers_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                          int64_t lda, const int32_t* cols, int K, const double* zs,
                          const int32_t* zcols, const int32_t* dates, int64_t nd,
                          const double* rows, const int32_t* rows_idx, const int32_t* nrows,
                          double* layer_mean, int32_t* layer_cnt, double* port, double* scratch);
/* The series of every (column, return) over the evaluated dates in their order (KKT:331-339,
 * 371): cum_layer [nd][K][3][10] the cumulative sum of layer_mean, cum_port [nd][K][3] that of
 * port -- a NaN entry stays NaN and the running sum carries on (pandas cumsum) -- and
 * ls [nd][K][3][5], ls[l - 1] = cum[10 - l + 1] - cum[l] for l = 1..5.  The per-year IR of the
 * screen is afm_screen_summary_f64's.  K >= 1, K * 18 < 2^31. */
int afm_screen_layer_series_f64(afm_ctx* ctx, int64_t nd, int K, const double* layer_mean,
                                const double* port, double* cum_layer, double* ls,
                                double* cum_port);

#ifdef __cplusplus
}
#endif

#endif /* AFM_SCREEN_LAYERS_H */
