/*
 * toucan_align.h - C ABI of the prosody cloner's kernels in libtoucan_hip.so (csrc/align.hip): the parts of the reference's
 * UtteranceCloner.extract_prosody (InferenceInterfaces/UtteranceCloner.py:46-145) that are not dense products.  Same conventions
 * as toucan_tts.h (device pointers owned by the caller, time-major packed rows, one hipStream_t per call, 0 or a negative
 * TTS_E_* code, tts_last_error()); the dense products of this path are tts_conv1d calls declared there.  The only caller is the
 * build's own Python host (ims-toucan-prosody-variance_amd/align.py, via ctypes: capi.ALIGN_PROTOTYPES).
 */
#ifndef TOUCAN_ALIGN_H
#define TOUCAN_ALIGN_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prosody cloner: Aligner, MAS durations, energy and pitch per token (UtteranceCloner.extract_prosody, UtteranceCloner.py:46-145) ----
 * The five Conv1d layers, the LSTM input projection (BatchNorm 5 and both LSTM biases folded in) and the output Linear run through
 * tts_conv1d in fp32 (ims-toucan-prosody-variance_amd/align.py packs them); these five entries are the rest (csrc/align.hip).  Every
 * entry computes an utterance in an order that depends on that utterance alone: a batch equals its utterances run one by one. */

/* y = max(x, 0) * scale[c] + shift[c]: ReLU, then BatchNorm1d in eval mode.  BatchNormConv.forward, Aligner.py:28-34. */
int tts_relu_affine(const float* x, int32_t ldx, float* y, int32_t ldy, int32_t rows, int32_t c, const float* scale, const float* shift,
                    tts_stream_t stream);
/* One time step of torch.nn.LSTM(bidirectional=True) with zero initial state over a ragged packed batch (Aligner.py:56,67-70 with
 * pack_padded_sequence): direction 0 processes row seq_begin[b] + step, direction 1 row seq_begin[b] + seq_len[b] - 1 - step;
 * utterances with seq_len[b] <= step are left alone.  xproj [rows, ldx >= 8*hidden]: the input projection plus both biases,
 * columns [direction][gate i, f, g, o][hidden].  w_hh_blk [2][hidden/4][hidden/16][16][16]: weight_hh_l0 / _reverse blocked per
 * slice s of 4 hidden units, w_hh_blk[d][s][kk][kg][g*4 + u] = W_hh[d][g*hidden + 4s + u][kg*hidden/16 + kk] (align.py packs it).  State
 * [batch][2][hidden], read from h_in / c_in (not read at step 0) and written to h_out / c_out (distinct buffers: the caller swaps
 * them between steps).  y [rows, ldy >= 2*hidden]: h of direction d in columns d*hidden ... .  hidden 256 or 512. */
int tts_lstm_recurrence(const float* xproj, int32_t ldx, const float* w_hh_blk, const float* h_in, const float* c_in, float* h_out, float* c_out,
                        float* y, int32_t ldy, const int32_t* seq_begin, const int32_t* seq_len, int32_t batch, int32_t hidden, int32_t step,
                        tts_stream_t stream);
/* Per-token durations of the full text, one workgroup per utterance: the token columns ids[id_begin[b] ...] (n_ids[b] of them) of
 * the logits rows frame_begin[b] ... (n_frames[b]) -> binarize_alignment (MAS: log(p + max|p| + 1), ties to j-1, row-0 quirk;
 * Aligner.py:202-234) -> DurationCalculator (DurationCalculator.py:17-31) -> zeros re-inserted at the word boundaries and the
 * 3/5 - 2/5 repair of repeated phonemes (UtteranceCloner.py:95-131).  flags [full text]: bit 0 word boundary, bit 1 same feature
 * vector as the previous token; n_full[b] tokens of which exactly n_ids[b] are not boundaries.  Decision bits: ceil(n_ids/64)
 * 64-bit words per frame, in LDS (up to lds_words words) when scratch_off[b] < 0, else in scratch + scratch_off[b].  An utterance
 * that fits neither gets durations -1.  max_ids: the largest n_ids (<= 8192).  durations int32 [sum n_full]. */
int tts_mas_durations(const float* logits, int32_t ld, const int32_t* frame_begin, const int32_t* n_frames, const int32_t* ids,
                      const int32_t* id_begin, const int32_t* n_ids, const int32_t* flags, const int32_t* full_begin, const int32_t* n_full,
                      const int64_t* scratch_off, uint64_t* scratch, int32_t batch, int32_t max_ids, int32_t lds_words, int32_t* durations,
                      tts_stream_t stream);
/* y[r] = sqrt(max(sum_c x[r, c]^2 + x[r, bins + c]^2, 1e-10)): frame energy of a spectrum stored as [re | im].
 * EnergyCalculator.py:68-71. */
int tts_frame_energy(const float* x, int32_t ldx, int32_t bins, float* y, int32_t rows, tts_stream_t stream);
/* Token averages over the durations, divided by the mean of the utterance's nonzero averages.  mode 0: mean of every frame
 * (EnergyCalculator._average_by_duration, :73-84, and norm_by_average, :61-64); mode 1: mean of the frames > 0
 * (PitchCalculator._average_by_duration, :106-117, and :56-58).  keep[k] == 0 zeroes token k.  x: frame values, utterance b at
 * x[frame_begin[b] ...] (n_frames[b]); durations / keep / out: [sum n_full], utterance b at full_begin[b].  max_full: the largest
 * n_full (<= 16384). */
int tts_token_average(const float* x, const int32_t* frame_begin, const int32_t* n_frames, const int32_t* durations, const int32_t* keep,
                      const int32_t* full_begin, const int32_t* n_full, int32_t batch, int32_t max_full, int32_t mode, float* out,
                      tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_ALIGN_H */
