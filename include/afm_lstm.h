/* afm_lstm.h -- ensembles of stacked LSTMs on the MI355X engine: the reference's
 * LSTM(H1, return_sequences) -> LSTM(H2) -> Dense(1) fitted with Adam on MSE without shuffling
 * (KKT:709-789), M of them side by side.  Conventions as in afm.h (device buffers, status
 * returns, afm_last_error()).
 *
 * The algorithm is pinned here and restated in numpy by tests/lstm_ref.py.  All values are fp64,
 * every operator below is one IEEE operation (no FMA contraction) except the sums of the matrix
 * products, which run on v_mfma_f64_16x16x4_f64 in the kernels' own order of addition: a function
 * of (T, d, H1, H2, nb) only -- never of the grid, of M, of the rows of a forward call or of a
 * work-split option -- and without floating-point atomics, so two runs agree bit for bit.
 *
 * Network: sequences of T steps with d inputs per step, hidden widths H1 and H2, one output.  The
 * parameters of one model are one flat vector theta[P] in the order
 *     K1[d + H1][4 H1]   rows 0..d-1: Keras's input kernel, the rest: its recurrent kernel
 *     b1[4 H1]
 *     K2[H1 + H2][4 H2]
 *     b2[4 H2]
 *     w[H2]
 *     b3
 * with the column blocks of width H in Keras's gate order i, f, g, o;
 * P = (d + H1) 4 H1 + 4 H1 + (H1 + H2) 4 H2 + 4 H2 + H2 + 1 = afm_lstm_param_count(d, H1, H2)
 * (121,301 at d = 1, H1 = H2 = 100, Keras's count).
 *
 * One layer step, from h_0 = c_0 = 0:
 *     a_t = [x_t | h_(t-1)]          z = a_t K + b       (the d + H terms of a sum padded to a
 *                                                          multiple of 4 with zero operands)
 *     i = sig(z_i)   f = sig(z_f)   g = tanh(z_g)   o = sig(z_o)
 *     c_t = f * c_(t-1) + i * g      h_t = o * tanh(c_t)
 * Layer 2's x_t is layer 1's h_t.  F = w . h2_T + b3.
 * sig(z) = 1.0 / (1.0 + exp(-z)); exp and tanh are the device math library's fp64 functions
 * (afm_lstm_act_f64 evaluates the kernels' own two device functions).
 *
 * Loss and backward of a batch of nb rows: dF = (F - y) * (2.0 / nb); g_w = h2_T' dF, g_b3 = sum
 * dF.  Per layer, for t = T..1, with dh_next = dc_next = 0 at t = T and tc = tanh(c_t):
 *     dh = dh_in_t + dh_next
 *     do = dh * tc
 *     dc = (dh * o) * (1.0 - tc * tc) + dc_next
 *     di = dc * g      dg = dc * i      df = dc * c_(t-1)      dc_next = dc * f
 *     dz = [ (di * i) * (1.0 - i) | (df * f) * (1.0 - f) | dg * (1.0 - g * g) | (do * o) * (1.0 - o) ]
 *     g_K += a_t' dz      g_b += sum over the rows of dz      [dx_t | dh_next] = dz K'
 * Layer 2's dh_in_T = dF (x) w and its other dh_in_t are 0.0; layer 1's dh_in_t is layer 2's dx_t.
 * The sums of g_K, g_b, g_w and g_b3 run over (t ascending, row ascending).
 *
 * Adam is exactly the recurrence of afm_mlp.h (b1p, b2p, lr_t, m, v, theta; one state per model).
 * The rows [0, n_train) train in that order (no shuffling); a short last batch is a batch of its
 * own size; an epoch is ceil(n_train / batch) steps from row 0.
 *
 * Design: X is [T][d][n_pad] -- one plane per (step, input), the planes afm_gbt_values_f64 writes
 * -- and y is [n_pad], n_pad a multiple of 64.  With d = 1 the [p][n_pad] design of afm_mlp.h is
 * this layout with T = p.  The cells of rows outside a call's range never reach a result: masked
 * rows (the end of a 16-row tile) load 0.0 and get dF = 0.
 *
 * Out of scope: dropout (Keras's mask stream cannot be reproduced; at prediction it is the
 * identity), shuffling, other optimisers, more than two recurrent layers, GRU and bidirectional
 * layers, the multi-GPU pipeline, fp32 or lower precision, a register-resident kernel specialised
 * to one shape.
 */
#ifndef AFM_LSTM_H
#define AFM_LSTM_H

#include "afm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AFM_LSTM_MAX_STEPS 256
#define AFM_LSTM_MAX_INPUTS 64
#define AFM_LSTM_MAX_HIDDEN 128
#define AFM_LSTM_MAX_MODELS 64
#define AFM_LSTM_MAX_BATCH 1024
#define AFM_LSTM_MAX_EPOCHS 4096

/* Common argument rules (AFM_E_ARG, nothing is launched): T outside 1..AFM_LSTM_MAX_STEPS; d
 * outside 1..AFM_LSTM_MAX_INPUTS; h1 or h2 not a multiple of 4 in 4..AFM_LSTM_MAX_HIDDEN; M
 * outside 1..AFM_LSTM_MAX_MODELS; n_pad < 64 or not a multiple of 64; a null buffer that is not
 * marked optional; a buffer that is not 16-byte aligned. */

/* P of the header comment.  Negative (afm_last_error() set) on bad d, h1, h2. */
int64_t afm_lstm_param_count(int d, int h1, int h2);

/* Bytes of the scratch of afm_lstm_fit_f64 / afm_lstm_grad_f64: the device copy of lr, and per
 * model the Adam moments m and v, the step state, and the gates, cell states and hidden states of
 * every (step, row) of one batch: about 8 * T * batch * 7 * (h1 + h2) bytes per model.  Negative
 * (afm_last_error() set) on bad T, d, h1, h2, M or batch (outside 1..AFM_LSTM_MAX_BATCH). */
int64_t afm_lstm_scratch_bytes(int T, int d, int h1, int h2, int M, int batch);

/* M fits side by side: `epochs` epochs of Adam steps on the rows [0, n_train).  Every launch of
 * every step and epoch is enqueued on the context's stream without a host synchronisation.  theta
 * [M][P]: in = the initial parameters, out = the fitted ones.  lr [M]: HOST doubles, one learning
 * rate per model.
 *
 * evals [M][epochs][2][6] = {n, sum F, sum y, sum F^2, sum y^2, sum F y} per epoch as in
 * afm_mlp.h: slot 0 over the training rows with the predictions each step made before its update,
 * slot 1 over the eval rows [n_train, n_train + n_eval) with the parameters at the end of the
 * epoch, all zero when n_eval = 0.  snaps [M][epochs][P] (optional): the parameters at the end of
 * each epoch.  scratch: afm_lstm_scratch_bytes(T, d, h1, h2, M, batch) bytes.
 *
 * The results are the same bits whatever the context option "lstm_rows_per_wg" is, and for a
 * model alone or inside any ensemble.
 *
 * No launch waits for the host.  The one transfer is the copy of lr[M] (hipMemcpyAsync from the
 * caller's pageable memory) at the start of the call: the runtime may hold the calling thread in
 * it until earlier work of the stream has drained; lr may be freed when the call returns.
 *
 * Also AFM_E_ARG: batch outside 1..AFM_LSTM_MAX_BATCH; epochs outside 1..AFM_LSTM_MAX_EPOCHS;
 * n_train < 1, n_eval < 0 or n_train + n_eval > n_pad; an lr[m] or eps that is not finite and
 * > 0; beta1 or beta2 outside [0, 1). */
int afm_lstm_fit_f64(afm_ctx* ctx, const double* X, const double* y, int64_t n_pad,
                     int64_t n_train, int64_t n_eval, int T, int d, int h1, int h2, int M,
                     double* theta, const double* lr, double beta1, double beta2, double eps,
                     int batch, int epochs, double* evals, double* snaps, double* scratch);

/* The gradient of the mean squared error of the one batch [i0, i0 + nb) for every model -- grad
 * [M][P], in the theta order -- and (optional) its predictions F [M][n_pad] (the cells [i0, i0 +
 * nb) of every model; the others are not touched), from the kernels the fit runs, without an
 * update.  scratch: afm_lstm_scratch_bytes(T, d, h1, h2, M, nb) bytes.  Also AFM_E_ARG: nb
 * outside 1..AFM_LSTM_MAX_BATCH; i0 < 0 or i0 + nb > n_pad. */
int afm_lstm_grad_f64(afm_ctx* ctx, const double* X, const double* y, int64_t n_pad, int64_t i0,
                      int nb, int T, int d, int h1, int h2, int M, const double* theta,
                      double* grad, double* F, double* scratch);

/* out[m][i] = F_m(x_i) for i in [i0, i0 + n), out [M][n_pad]; the other cells are not touched.  A
 * row's value does not depend on i0, n or the rows around it.  AFM_E_ARG: i0 < 0, n < 0 or i0 + n
 * > n_pad; n = 0 returns at once. */
int afm_lstm_forward_f64(afm_ctx* ctx, const double* X, int64_t n_pad, int64_t i0, int64_t n,
                         int T, int d, int h1, int h2, int M, const double* theta, double* out);

/* out[k] = sig(x[k]) (kind 0) or tanh(x[k]) (kind 1) for k in [0, n): the device functions the
 * recurrent kernels call.  AFM_E_ARG: kind outside 0..1; n < 0; n = 0 returns at once. */
int afm_lstm_act_f64(afm_ctx* ctx, int kind, const double* x, int64_t n, double* out);

#ifdef __cplusplus
}
#endif

#endif /* AFM_LSTM_H */
