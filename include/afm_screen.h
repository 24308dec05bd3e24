/* afm_screen.h -- factor screening on the MI355X engine: the per-date Pearson IC of K factor
 * columns against return_1 / return_2 / return_5 in one pass over the panel, and the per-year IR
 * and whole-sample summary of every column.  Conventions as in afm.h (device buffers, calendar
 * grids, status returns, afm_last_error()).
 *
 * The reference screens one column at a time: AlphaSignalAnalyzer(df_train_x[['d11']], 'd11',
 * df_train[['close_price']]).run() (KKT:465, 472), whose IC is DataFrame.corr(method='pearson')
 * per date (KKT:342-349) and whose IR is mean / std of the ICs per year (KKT:351-354).  All
 * columns of one frame share the rows, the forward returns and the per-date demeans, so those
 * are prepared once (afm_fwd_returns_f64, afm_xs_prepare_f64 with a signal plane that marks the
 * rows) and these two entry points evaluate every column on them.  The rank (Spearman) IC of the
 * same columns is afm_rankic.h's; the decile layers, long-short spreads and top-10 backtest of
 * every column on the same preparation (KKT:324-375) are afm_screen_layers.h's.
 */
#ifndef AFM_SCREEN_H
#define AFM_SCREEN_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ic [nd][K][3]: for evaluated date i (t = dates[i], DEVICE int32 [nd], any order), column k and
 * return q the pandas nancorr of (return q, factor k) over the date's compacted rows in row
 * order -- rows [4][T][lda] (planes 1..3: the demeaned returns), rows_idx [T][lda], nrows [T] as
 * afm_xs_prepare_f64 wrote them.  Factor k of row e is plane base + cols[k] * col_stride
 * ([T][lda], cols DEVICE int32 [K], repeats allowed) at [t][rows_idx[t][e]]; with zs (the
 * [..][lda][2] = {mu, 1/sd} table of afm_zstats_finalize_f64) it is z = (x - mu) * (1/sd) of row
 * zcols[k] (DEVICE int32 [K]; NULL = row k), zs == NULL: the raw value.  A row is skipped for a
 * (k, q) when its factor value or its return is not finite; the IC is NaN where no row is left
 * or either variance is 0.  Only the rows [0, nd) of ic are written.  K >= 1, lda % 64 == 0,
 * nd * ceil(K / 64) < 2^31. */
int afm_screen_ic_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                      int64_t lda, const int32_t* cols, int K, const double* zs,
                      const int32_t* zcols, const int32_t* dates, int64_t nd, const double* rows,
                      const int32_t* rows_idx, const int32_t* nrows, double* ic);
/* Over the non-NaN ICs of every (column, return) -- the reference's .stack() drops NaN --
 * stats [K][3][5] = {n, mean, std (ddof = 1), ir = mean / std, t = ir * sqrt(n)} of the whole
 * sample, and ir_year [nyears][K][3] = mean / std of the ICs of the dates with year[i] ==
 * year0 + y (KKT:353; the dates of a year need not be contiguous; NaN for a year with fewer than
 * two ICs).  numpy's sums: the buffered pairwise sum and the two-pass std of pandas' nanops.
 * year DEVICE int32 [nd]; 0 <= nyears <= 320; scratch [K][3][2][nd] doubles. */
int afm_screen_summary_f64(afm_ctx* ctx, const double* ic, int64_t nd, int K, const int32_t* year,
                           int nyears, int year0, double* stats, double* ir_year,
                           double* scratch);

#ifdef __cplusplus
}
#endif

#endif /* AFM_SCREEN_H */
