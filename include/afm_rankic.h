/* afm_rankic.h -- the rank (Spearman) IC on the MI355X engine: DataFrame.corr(method='spearman')
 * per date, what AlphaSignalAnalyzer computes with corr_method = 'spearman' (KKT:286, 344-345), for
 * one signal or for the K columns of a factor screen.  Conventions as in afm.h (device buffers,
 * calendar grids, status returns, afm_last_error()); rows / rows_idx / nrows are what
 * afm_xs_prepare_f64 wrote, the column arguments those of afm_screen_ic_f64 (afm_screen.h), and
 * afm_screen_summary_f64 / afm_xs_series_f64 take the rank ICs as they are.
 *
 * pandas' nancorr_spearman for a pair (factor f, return r) on one date: fx = isfinite(f), fy =
 * isfinite(r), m = fx & fy, nobs = count(m) (0: NaN).  Average-tie ascending ranks (-0.0 ties with
 * 0.0; NaN takes no rank): when fx == fy on every row, each column ranked over its non-NaN rows and
 * restricted to m (+-inf rows keep their places in the ranking), else both re-ranked over m.
 * With mean = (nobs + 1) / 2 the sums of (rx - mean)(ry - mean), (rx - mean)^2, (ry - mean)^2 are
 * exact in any order (half-integers, n <= 32768: integers below 2^53 in doubled units), and
 * IC = sumxy / sqrt(sumxx * sumyy), NaN when the root is 0.
 */
#ifndef AFM_RANKIC_H
#define AFM_RANKIC_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int64 words of scratch the two entry points below need at this lda: 0 when every date sorts in
 * LDS (lda <= 16384), else room for the sorted chunks of the dates in flight.  Negative: lda is
 * not a positive multiple of 64 up to 32768. */
int64_t afm_rank_scratch_words(int64_t lda);
/* The doubled average ranks of the three demeaned returns (planes 1..3 of rows [4][T][lda]) over
 * the compacted rows of each evaluated date t = dates[i] (DEVICE int32 [nd], any order):
 * rrank [3][T][lda] int32, 2 * rank of row e at [q][t][e], and rsum [T][3] int64, the sum of
 * (2 * rank - (n + 1))^2 over the date's rows, or -1 when return q is not finite on every row of
 * the date (the date then takes the masked path of afm_screen_rank_ic_f64).  Only the evaluated
 * dates are written.  scratch: afm_rank_scratch_words(lda) words (may be NULL when that is 0).
 * lda % 64 == 0, lda <= 32768, nd * 3 < 2^31. */
int afm_rank_returns_f64(afm_ctx* ctx, int64_t T, int64_t lda, const int32_t* dates, int64_t nd,
                         const double* rows, const int32_t* nrows, int32_t* rrank, int64_t* rsum,
                         uint64_t* scratch);
/* ic [nd][K][3]: the Spearman IC of column k against return q on date dates[i] -- the arguments of
 * afm_screen_ic_f64, then rrank / rsum as afm_rank_returns_f64 wrote them for (at least) these
 * dates, and the scratch.  Only the rows [0, nd) of ic are written.  K >= 1, lda % 64 == 0,
 * lda <= 32768, nd * K < 2^31. */
int afm_screen_rank_ic_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                           int64_t lda, const int32_t* cols, int K, const double* zs,
                           const int32_t* zcols, const int32_t* dates, int64_t nd,
                           const double* rows, const int32_t* rows_idx, const int32_t* nrows,
                           const int32_t* rrank, const int64_t* rsum, uint64_t* scratch,
                           double* ic);

#ifdef __cplusplus
}
#endif

#endif /* AFM_RANKIC_H */
