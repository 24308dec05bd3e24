/* afm_seams.h -- fused launches for the serial seams of the pipeline step: each entry point does
 * in ONE launch what a run of small dependent launches of afm.h does, and leaves bitwise the same
 * results (the same additions in the same order; only which launch performs them changes).
 * Conventions as in afm.h (device buffers, calendar grids, status returns, afm_last_error()).
 */
#ifndef AFM_SEAMS_H
#define AFM_SEAMS_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The pooled-Gram leaves of afm_zpool_f64, leaves [nrb][c2 * c1][part] (nchunk = c2 * c1), to the
 * asset-block partials out [nblk][part]: per element the fixed trees of
 *   afm_gram_tree_f64(p, leaves, nrb * c2 * c1, c1, 0, a);
 *   afm_gram_tree_f64(p, a, nrb * c2, c2, 0, b);
 *   afm_gram_tree_f64(p, b, nrb, rb_per_blk, 0, out);
 * (the last block may be short).  A block past the last row-block is written as zeros: out needs
 * no clearing.  1 <= c1, c2, rb_per_blk <= 32, c2 * rb_per_blk <= 64, nblk * rb_per_blk >= nrb. */
int afm_gram_tree3_f64(afm_ctx* ctx, int p, const double* leaves, int nrb, int c1, int c2,
                       int rb_per_blk, int nblk, double* out);
/* The block level of the pooled Gram: gram [p+2][p+2] = the final tree over blocks [nblk][part]
 * (afm_gram_tree_f64(p, blocks, nblk, nblk, 1, gram)); with te_leaves [nte][part] (may be NULL)
 * also te_gram = their final tree and gram += te_gram (afm_vec_add_f64): the train_end date
 * counted twice.  1 <= nblk, nte <= 32. */
int afm_gram_final_f64(afm_ctx* ctx, int p, const double* blocks, int nblk,
                       const double* te_leaves, int nte, double* gram, double* te_gram);
/* afm_ols_solve_f64 on the raw-moment Grams of afm_gram_tree_f64(p, parts, nseg * per, per, 1,
 * gram), without that launch: segment s is solved from the tree over its partials
 * parts [nseg][per][part], merged while they are loaded.  shift [nseg][p+2] as for
 * afm_ols_solve_f64 (zeros for raw moments).  1 <= p <= 106, 1 <= per <= 32. */
int afm_ols_solve_parts_f64(afm_ctx* ctx, const double* parts, int per, const double* shift, int p,
                            int64_t nseg, double tol, double* beta, double* nobs, int32_t* rank);
/* afm_factors_f64, then afm_drop_last_obs_bits of both masks, with the masks in one launch:
 * alldf_bits = nanfree_bits and frows_bits = finite_bits without each asset's last present day.
 * Every bit-word buffer [ceil(T/64)][lda]; finite_bits is required here. */
int afm_factors_rows_f64(afm_ctx* ctx, int64_t T, int64_t A, int64_t lda, const double* close,
                         const double* volume, const double* ret1d, const double* excess,
                         const uint64_t* valid_bits, double* out, uint64_t* nanfree_bits,
                         uint64_t* finite_bits, uint64_t* alldf_bits, uint64_t* frows_bits);
/* afm_zstats_finalize_f64, then afm_row_bits(nch, lda, rows, NULL, asset_ok, t0, t1, out), in one
 * launch. */
int afm_zstats_rows_f64(afm_ctx* ctx, const double* mu, const double* sd, int K, int64_t lda,
                        double* zs, int32_t* asset_ok, int64_t nch, const uint64_t* rows,
                        int64_t t0, int64_t t1, uint64_t* out);

#ifdef __cplusplus
}
#endif

#endif /* AFM_SEAMS_H */
