/* afm_mv.h -- the mean-variance entry points of the MI355X engine: the rebalance and the one-book
 * weight solve of afm.h with an expected-return term.  Conventions as in afm.h (device buffers,
 * calendar grids, status returns, afm_last_error()).
 *
 * Per book the solve is
 *     minimise  1/2 w'S w - gamma * s * mu'w    subject to  sum w = 1,  lo <= w <= hi
 * with S the book's pairwise-complete history covariance (as afm_rebalance_f64), gamma >= 0 the
 * risk tolerance, s = +1 for the long book and -1 for the short book (short weights are
 * magnitudes: its best names have the most negative expected return).  The optimum is exact
 * (primal active set, as the min-variance solve); a fully bound vertex is tested for optimality
 * and left by releasing one member at each bound.  gamma must be finite and >= 0 (AFM_E_ARG).
 *
 * The per-date book arrays (books, weights, upos) have a stride of 128 names per book, the
 * library's book-size cap.
 */
#ifndef AFM_MV_H
#define AFM_MV_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* afm_rebalance_f64 with the return term.  mu: [T][lda] plane of expected returns read at each
 * rebalance date (the prediction plane itself is the natural choice; a non-finite value counts as
 * 0), or NULL = each member's mean over its finite rows of the history window the covariance
 * reads.  Selection, k_out, books, upos, usize and the status codes are those of
 * afm_rebalance_f64; gamma == 0: bit-identical to afm_rebalance_f64. */
int afm_rebalance_mv_f64(afm_ctx* ctx, int64_t T, int64_t A, int64_t lda, const int32_t* dates,
                         int64_t nd, const double* pred, const uint64_t* trad_bits,
                         const double* hist, const uint64_t* hist_bits, int64_t h_t0,
                         int64_t h_t1, int64_t window, const double* close, const double* tmr,
                         int top_n, double lo, double hi, const double* mu, double gamma,
                         int32_t* k_out, int32_t* books, double* weights, double* sums,
                         int32_t* upos, int64_t* usize, int32_t* status);
/* One book (sign +1): afm_min_variance_weights_f64 with the return term.  mu: DEVICE [k] (a
 * non-finite value counts as 0), or NULL = the column means of R over their finite rows.
 * gamma == 0: bit-identical to afm_min_variance_weights_f64. */
int afm_mean_variance_weights_f64(afm_ctx* ctx, const double* R, int64_t rows, int64_t ld, int k,
                                  const double* mu, double gamma, double lo, double hi, double* w,
                                  double* cov, int32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* AFM_MV_H */
