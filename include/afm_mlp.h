/* afm_mlp.h -- ensembles of small dense networks on the MI355X engine: the reference's
 * Dense(128, relu) -> Dense(32, relu) -> Dense(1) fitted with Adam on the z-scored panel
 * (KKT:668-706), M of them side by side, one workgroup per network.  Conventions as in afm.h
 * (device buffers, status returns, afm_last_error()).
 *
 * The algorithm is pinned here and restated in numpy by tests/mlp_ref.py.  All values are fp64,
 * every operator below is one IEEE operation (no FMA contraction) except the sums of the layer
 * and gradient products, whose order of addition is the kernel's own: a function of the shapes
 * only (v_mfma_f64_16x16x4_f64 over a fixed tiling, no floating-point atomics), so two runs agree
 * bit for bit.
 *
 * Network: p inputs, hidden widths h1 and h2, one output.  The parameters of one model are one
 * flat vector theta[P] in the order W1[p][h1], b1[h1], W2[h1][h2], b2[h2], w3[h2], b3, P =
 * afm_mlp_param_count(p, h1, h2).  f(x) = w3 . relu(W2' relu(W1' x + b1) + b2) + b3 with relu(z)
 * = z > 0 ? z : 0, derivative z > 0.
 *
 * Design: X is [p][n_pad] (one plane per column, what afm_gbt_values_f64 writes), y is [n_pad].
 * The rows [0, n_train) train, in that order (no shuffling); the rows [n_train, n_train + n_eval)
 * are only evaluated; the cells of the rows >= n_train + n_eval never reach a result.
 *
 * One step: the batch is the rows [i, i + nb), nb = min(batch, n_train - i) -- a short last batch
 * is a batch of its own size.  Forward gives z1, a1, z2, a2, f; d = (f - y) * (2.0 / nb);
 * g_w3 = a2' d, g_b3 = sum d, d2 = (d (x) w3) . [z2 > 0], g_W2 = a1' d2, g_b2 = sum d2,
 * d1 = (d2 W2') . [z1 > 0], g_W1 = X' d1, g_b1 = sum d1.
 *
 * Adam in Keras's form, state b1p = b2p = 1.0 and m = v = 0 per model, each step
 *     b1p = b1p * beta1;  b2p = b2p * beta2
 *     lr_t = (lr * sqrt(1.0 - b2p)) / (1.0 - b1p)
 *     m = m + (g - m) * c1            c1 = 1.0 - beta1
 *     v = v + (g * g - v) * c2        c2 = 1.0 - beta2
 *     theta = theta - (lr_t * m) / (sqrt(v) + eps)
 *
 * An epoch is ceil(n_train / batch) steps from row 0.
 */
#ifndef AFM_MLP_H
#define AFM_MLP_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_MLP_MAX_COLS 64
#define AFM_MLP_MAX_HIDDEN 128
#define AFM_MLP_MAX_WIDTH_SUM 192
#define AFM_MLP_MAX_WEIGHTS 16384
#define AFM_MLP_MAX_MODELS 1024
#define AFM_MLP_MAX_BATCH 4096
#define AFM_MLP_MAX_EPOCHS 4096

/* Common argument rules (AFM_E_ARG, nothing is launched): p outside 1..AFM_MLP_MAX_COLS; h1 or h2
 * not a multiple of 16 in 16..AFM_MLP_MAX_HIDDEN; h1 + h2 > AFM_MLP_MAX_WIDTH_SUM or h1 * (p4 +
 * h2) > AFM_MLP_MAX_WEIGHTS, p4 = p rounded up to 4 (a model's parameters and one 16-row tile of
 * both activations share the 160 KiB of LDS of a compute unit); M outside
 * 1..AFM_MLP_MAX_MODELS; n_pad < 64 or not a multiple of 64; a null buffer that is not marked
 * optional; a buffer that is not 16-byte aligned. */

/* P = p h1 + h1 + h1 h2 + h2 + h2 + 1.  Negative (afm_last_error() set) on bad p, h1, h2. */
int64_t afm_mlp_param_count(int p, int h1, int h2);

/* Bytes of afm_mlp_fit_f64's scratch: per model the Adam moments m and v, the step state and the
 * activations of one batch.  Negative (afm_last_error() set) on bad p, h1, h2, M or batch
 * (outside 1..AFM_MLP_MAX_BATCH). */
int64_t afm_mlp_scratch_bytes(int p, int h1, int h2, int M, int batch);

/* M fits side by side, enqueued without a host synchronisation: `epochs` epochs of Adam steps on
 * the rows [0, n_train).  theta [M][P]: in = the initial parameters, out = the fitted ones.  lr
 * [M]: HOST doubles, one learning rate per model.
 *
 * evals [M][epochs][2][6] = {n, sum F, sum y, sum F^2, sum y^2, sum F y} per epoch: slot 0 over
 * the training rows with the predictions each step made before its update (what Keras reports as
 * `loss`), slot 1 over the eval rows with the parameters at the end of the epoch (`val_loss`),
 * all zero when n_eval = 0.  snaps [M][epochs][P] (optional): the parameters at the end of each
 * epoch.  scratch: afm_mlp_scratch_bytes(p, h1, h2, M, batch) bytes.
 *
 * A launch runs at most S steps of every model and leaves theta, m, v, b1p, b2p and the running
 * moments in theta / scratch for the next launch; S is the context option "mlp_steps_per_launch".
 * The results are the same bits whatever S is.
 *
 * Also AFM_E_ARG: batch outside 1..AFM_MLP_MAX_BATCH; epochs outside 1..AFM_MLP_MAX_EPOCHS;
 * n_train < 1, n_eval < 0 or n_train + n_eval > n_pad; an lr[m] or eps that is not finite and
 * > 0; beta1 or beta2 outside [0, 1). */
int afm_mlp_fit_f64(afm_ctx* ctx, const double* X, const double* y, int64_t n_pad,
                    int64_t n_train, int64_t n_eval, int p, int h1, int h2, int M, double* theta,
                    const double* lr, double beta1, double beta2, double eps, int batch,
                    int epochs, double* evals, double* snaps, double* scratch);

/* out[m][i] = f_m(x_i) for i in [i0, i0 + n), out [M][n_pad]; the other cells are not touched.  A
 * row's value does not depend on i0, n or the rows around it.  AFM_E_ARG: i0 < 0, n < 0 or i0 + n
 * > n_pad; n = 0 returns at once. */
int afm_mlp_forward_f64(afm_ctx* ctx, const double* X, int64_t n_pad, int64_t i0, int64_t n,
                        int p, int h1, int h2, int M, const double* theta, double* out);

#ifdef __cplusplus
}
#endif

#endif /* AFM_MLP_H */
