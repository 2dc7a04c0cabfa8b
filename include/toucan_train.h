/*
 * toucan_train.h - C ABI of the aligner's on-line fine-tuning in libtoucan_hip.so (csrc/train.hip): the five SGD steps of CTC
 * training that the reference's UtteranceCloner.extract_prosody runs on the utterance it is about to align
 * (InferenceInterfaces/UtteranceCloner.py:75-94; the model: AutoAligner/Aligner.py:18-75).  Same conventions as toucan_tts.h (device
 * pointers owned by the caller, time-major rows, one hipStream_t per call, 0 or a negative TTS_E_* code, tts_last_error()).  The
 * only caller is the build's own Python host (ims-toucan-prosody-variance_amd/finetune.py, via ctypes: capi.TRAIN_PROTOTYPES).
 *
 * One utterance per call.  Everything is fp32 (the CTC recursions fp64) and deterministic: fixed accumulation orders, no atomics,
 * and no kernel waits on another workgroup - the recurrences are one launch per time step.
 */
#ifndef TOUCAN_TRAIN_H
#define TOUCAN_TRAIN_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* C = op(A) * op(B) [+ bias] [+ C] on row-major operands with leading dimensions, on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32: every element is one k-ordered fma chain).  op: 0 NN (A [M, K], B [K, N]), 1 NT (A [M, K], B [N, K]),
 * 2 TN (A [K, M], B [K, N]).  bias (may be null): one value per column of C.  accumulate != 0 adds the product to C.  Any
 * M, N, K >= 0 (K == 0 gives the bias or zero); rows of an operand may overlap (lda < its width: the k 3 convolution as one product
 * over a padded activation).  Each 64 x 64 tile of C reduces K in one workgroup. */
#define TTS_GEMM_NN 0
#define TTS_GEMM_NT 1
#define TTS_GEMM_TN 2
int tts_gemm_f32(int32_t op, const float* a, int32_t lda, const float* b, int32_t ldb, float* c, int32_t ldc, const float* bias, int32_t m,
                 int32_t n, int32_t k, int32_t accumulate, tts_stream_t stream);

/* BatchNormConv in training mode after the conv (Aligner.py:28-34) and the Dropout(0.5) that follows it (:47): r = max(z, 0);
 * mean and biased variance of r over the t frames per channel (two passes); y = ((r - mean) * istd * gamma + beta) * 2 * mask,
 * istd = 1 / sqrt(var + eps).  mask [t, c] bytes (0 / 1), null: no dropout.  save_mean / save_istd [c] are written;
 * running_mean / running_var [c] (null: left alone) move by `momentum`, the variance by the unbiased one (t >= 2).
 * c a multiple of 64. */
int tts_bn_train_forward(const float* z, int32_t ldz, const uint8_t* mask, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float* y, int32_t ldy, float* save_mean, float* save_istd, int32_t t, int32_t c, float eps,
                         float momentum, tts_stream_t stream);
/* Its backward: g = dy * 2 * mask; dbeta = sum_t g; dgamma = sum_t g * xhat; dz = [z > 0] * gamma * istd * (g - mean_t g -
 * xhat * mean_t (g * xhat)), xhat recomputed from z and the saved statistics.  dz must not alias dy. */
int tts_bn_train_backward(const float* dy, int32_t lddy, const float* z, int32_t ldz, const uint8_t* mask, const float* gamma,
                          const float* save_mean, const float* save_istd, float* dz, int32_t lddz, float* dgamma, float* dbeta, int32_t t,
                          int32_t c, tts_stream_t stream);
/* scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale (formed in fp64): eval BatchNorm as the operands
 * of tts_relu_affine. */
int tts_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float* scale,
                       float* shift, int32_t c, float eps, tts_stream_t stream);

/* One time step of torch.nn.LSTM(bidirectional=True), zero initial state, of one utterance of t frames, keeping what the backward
 * pass needs.  Direction 0 processes row `step`, direction 1 row t - 1 - step.  xproj [t, ldx >= 8*hidden]: the input projection,
 * columns [direction][gate i, f, g, o][hidden]; b_ih / b_hh [2][4*hidden] are added here.  w_hh [2][4*hidden][hidden]: weight_hh_l0 /
 * _reverse as torch stores them.  y [t, ldy >= 2*hidden] receives h (and is read for the previous step's h); gates [t][2][4*hidden]
 * the activated gates; cseq [t][2][hidden] the cell state.  hidden 512. */
int tts_lstm_train_step(const float* xproj, int32_t ldx, const float* w_hh, const float* b_ih, const float* b_hh, float* y, int32_t ldy,
                        float* gates, float* cseq, int32_t t, int32_t hidden, int32_t step, tts_stream_t stream);
/* One step of its backward pass, to be called with step = t - 1 down to 0.  dy [t, lddy >= 2*hidden]: the gradient of y; the
 * recurrent part w_hh^T * dgates of the step called just before is added here.  dgates [t][2][4*hidden] receives the gradient of
 * the pre-activation gates of this step's rows; dc [2][hidden] carries the cell gradient between calls (not read at step t - 1). */
int tts_lstm_backward_step(const float* dy, int32_t lddy, const float* w_hh, const float* gates, const float* cseq, float* dgates, float* dc,
                           int32_t t, int32_t hidden, int32_t step, tts_stream_t stream);

/* CTCLoss(blank, zero_infinity=True), reduction "mean" at batch 1, of log_softmax(logits) and its gradient with respect to the
 * logits, one workgroup: loss[0] = -log p(targets | logits) / n_targets; grad [t, ldg] = (softmax - posterior) / n_targets.  The
 * log-softmax is fp32 (as the reference's); the forward and backward variables over the 2n+1 extended states are fp64.  An
 * infeasible alignment gives loss 0 and a zero gradient.  Scratch: alpha [t][2*n_targets + 1] fp64, lp [t][n_symbols] fp32.
 * 1 <= n_targets <= TTS_CTC_GRAD_MAX_TARGETS, n_symbols <= 256; target ids in [0, n_symbols) and not the blank (else NaN). */
#define TTS_CTC_GRAD_MAX_TARGETS 768
int tts_ctc_grad(const float* logits, int32_t ld, int32_t n_symbols, int32_t t, const int32_t* targets, int32_t n_targets, int32_t blank,
                 double* alpha, float* lp, float* loss, float* grad, int32_t ldg, tts_stream_t stream);

/* out[j] (and out2[j] if not null) = sum_r x[r, j], rows added in a fixed order. */
int tts_col_sum(const float* x, int32_t ldx, int32_t rows, int32_t cols, float* out, float* out2, tts_stream_t stream);
/* norm[0] = sqrt(sum_i x[i]^2): fp64 partial sums per workgroup (partials: TTS_SUMSQ_PARTIALS doubles of scratch), then one
 * workgroup adds them, both in a fixed order. */
#define TTS_SUMSQ_PARTIALS 256
int tts_sumsq(const float* x, int64_t n, double* partials, float* norm, tts_stream_t stream);
/* clip_grad_norm_ + SGD: p[i] -= lr * (g[i] * min(1, max_norm / (norm[0] + 1e-6))), the norm read from device memory. */
int tts_sgd_clip_update(float* p, const float* g, int64_t n, const float* norm, float max_norm, float lr, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_TRAIN_H */
