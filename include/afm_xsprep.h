/* afm_xsprep.h -- the stage in front of the factor screen on the MI355X engine: what a multi-factor
 * workflow does to a factor ACROSS THE SECURITIES OF ONE DATE before it is rated or regressed --
 * winsorise (median +- c MAD, or two quantiles), take out the group (sector) mean, standardise to
 * mean 0 and sd 1 -- for K columns and nd dates in one call.  Conventions as in afm.h (device
 * buffers, calendar grids, status returns, afm_last_error()).
 *
 * In pandas: df.groupby('date')[c].transform(...) per column, the missing cells of the column
 * dropped first.
 */
#ifndef AFM_XSPREP_H
#define AFM_XSPREP_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_XSPREP_WINSOR_NONE 0
#define AFM_XSPREP_WINSOR_MAD 1
#define AFM_XSPREP_WINSOR_QUANTILE 2
#define AFM_XSPREP_NEUTRALIZE 1    /* flags bit 0 */
#define AFM_XSPREP_STANDARDIZE 2   /* flags bit 1 */
#define AFM_XSPREP_MAX_GROUPS 256
#define AFM_XSPREP_INFO 7          /* doubles per (date, column) of info */

/* For evaluated date i (t = dates[i], DEVICE int32 [nd], any order) and column k: the arguments up
 * to nd are afm_screen_ic_f64's (without the unused `rows`) and the value x_e of a row e <
 * nrows[t] is the same double: plane base + cols[k] * col_stride at [t][rows_idx[t][e]], with zs
 * z = (x - mu) * (1/sd) of row zcols[k] (NULL = row k).
 *
 * A cell is missing for its own column when x_e is not finite and, with AFM_XSPREP_NEUTRALIZE, when
 * its group is outside [0, ngroups).  F = the rows that are not missing, n = |F|.  In this order:
 *   1. winsorise.  winsor = 0: lo = -inf, hi = +inf.  1: med = the median of F (the middle value,
 *      or (a + b) / 2 of the two middle ones), mad = the median of |x - med|, lo = med - p_lo * mad,
 *      hi = med + p_hi * mad (the caller passes c = n_mad * 1.4826 twice); mad == 0: no clipping
 *      (lo = -inf, hi = +inf).  2: lo, hi = numpy.quantile(F, p_lo), (F, p_hi), method 'linear':
 *      v = (n - 1) q, i = floor(v), g = v - i, a = s[i], b = s[min(i + 1, n - 1)], a + (b - a) g
 *      where g < 0.5, else b - (b - a)(1 - g).  w = min(max(x, lo), hi); n_lo, n_hi = the rows
 *      with x < lo, x > hi.  With n == 0, lo = hi = NaN in modes 1 and 2.
 *   2. neutralise (flags bit 0): g_e = groups[t * g_stride + rows_idx[t][e]] (g_stride = 0: one
 *      label per asset; lda: a [T][lda] plane), v = w - (the mean of w over the rows of F in the
 *      group); a group of one row gives exactly 0.  Off: v = w, groups may be NULL.
 *   3. standardise (flags bit 1): mu = sum v / n, sd = sqrt(sum (v - mu)^2 / (n - 1)), out =
 *      (v - mu) / sd; with n < 2 or sd zero or not finite every row of the item is NaN.  Off:
 *      out = v.
 * Plane k of the output is out + k * out_stride, [T][lda]: for an evaluated date the whole [lda]
 * row is written, the result on the assets of F and NaN on every other cell; the rows of other
 * dates are not touched.  info [nd][K][7] = {n, lo, hi, n_lo, n_hi, mu, sd}, mu and sd NaN without
 * bit 1 (mu also with n == 0, sd with n < 2).
 *
 * Order statistics are exact values: n, lo, hi, n_lo, n_hi and the output without flags are those
 * of numpy bit for bit (by value: a -0.0 may come out as 0.0).  The sums of steps 2 and 3 are
 * formed exactly -- every addend on a fixed-point grid of the item, 64-bit integer accumulators --
 * so they depend on no order: an item's output is a function of its column's values on the date's
 * rows and of their groups alone, bitwise the same whatever K, the position in cols, the other
 * columns and dates of the call.  The means are carried as double-double.
 *
 * AFM_E_ARG: K < 1; lda % 64 != 0 or lda > 32768; an unknown winsor mode or flag bit; mode 1 with
 * a p that is not finite or <= 0; mode 2 without 0 <= p_lo < p_hi <= 1; bit 0 with groups NULL or
 * ngroups outside 1..256; g_stride other than 0 or lda; out overlapping a plane it reads (cols is
 * copied to the host for this check: the call waits for the context's stream).  nd == 0 returns
 * AFM_OK at once. */
int afm_xs_preprocess_f64(afm_ctx* ctx, const double* base, int64_t col_stride, int64_t T,
                          int64_t lda, const int32_t* cols, int K, const double* zs,
                          const int32_t* zcols, const int32_t* dates, int64_t nd,
                          const int32_t* rows_idx, const int32_t* nrows, const int32_t* groups,
                          int64_t g_stride, int ngroups, int winsor, double p_lo, double p_hi,
                          int flags, double* out, int64_t out_stride, double* info);

#ifdef __cplusplus
}
#endif

#endif /* AFM_XSPREP_H */
