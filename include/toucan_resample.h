/*
 * toucan_resample.h - C ABI of the sample-rate converter in libtoucan_hip.so (csrc/resample.hip): band-limited resampling of a
 * ragged batch of waveforms by a rational factor, float32 or PCM16 out, with torchaudio.transforms.Resample's defaults (Hann
 * window, lowpass_filter_width 6, rolloff 0.99) - third party, PARITY UNPINNED: torchaudio is not available to compare against;
 * DESIGN.md section 13 holds the definition and tests/resample_ref.py its float64 restatement.  Same conventions as
 * toucan_pitch.h: device pointers owned by the caller, ragged packed batches, one hipStream_t per call, 0 or a negative TTS_E_*
 * code, tts_last_error(); an utterance's result depends on that utterance alone.  The build's own caller is
 * ims-toucan-prosody-variance_amd/resample.py (ctypes: capi.RESAMPLE_PROTOTYPES).
 *
 * The filter, for the caller who builds the table (in float64, rounded to float32 once):
 *     g = gcd(sr_in, sr_out), orig = sr_in / g, new = sr_out / g, base = min(orig, new) * 0.99,
 *     w = ceil(6 orig / base), K = 2 w + orig,
 *     t(p, j) = clip(((j - w) / orig - p / new) * base, -6, 6),
 *     k[p][j] = sinc(pi t) * cos^2(pi t / 12) * base / orig            (sinc(0) = 1),      p < new, j < K.
 * With x taken as 0 outside [0, n), output m = i new + p of an utterance of n samples is
 *     y[m] = sum_{j < K} k[p][j] * x[i orig + j - w],                                      m < ceil(new n / orig).
 * The same rate in and out is the table orig = new = 1, w = 0, k = {{1}}.
 */
#ifndef TOUCAN_RESAMPLE_H
#define TOUCAN_RESAMPLE_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_RESAMPLE_MAX_FACTOR 1024 /* the most orig and new may be: 24000 -> 44100 is 80 / 147, 44100 -> 16000 is 441 / 160 */
#define TTS_RESAMPLE_LDS_TABLE_BYTES 65536 /* a table up to this size is staged in LDS; a larger one is read through L2 */

/* One utterance of a launch.  The buffer holds the utterance's samples pos0 .. pos0 + n_held - 1 (pos0 = 0 for a whole utterance,
 * > 0 for the continuation of a streamed one); a sample the buffer does not hold counts as 0.  The launch writes the outputs
 * out_first .. out_first + out_count - 1 of the utterance to y[out_begin ...]. */
typedef struct TtsResampleSpan {
  int64_t in_begin;  /* first sample of the buffer in the packed input */
  int64_t n_held;    /* samples the buffer holds */
  int64_t pos0;      /* position of the buffer's first sample within the utterance */
  int64_t out_first; /* first output index */
  int64_t out_count; /* outputs to write */
  int64_t out_begin; /* where they go in the packed output */
} TtsResampleSpan;

/* Outputs one workgroup produces (consecutive ones of one utterance, from out_first on). */
int tts_resample_tile_outputs(void);

/* y = the filter above applied to every span.  table: float32 [K][new], TRANSPOSED - element j * new + p is k[p][j] - so that
 * neighbouring outputs read neighbouring coefficients.  spans [batch] and table on the device; max_out_count >= every
 * out_count.  pcm16 = 0: y is float32.  pcm16 = 1: y is int16, the reference's float2pcm (Utility/utils.py:20-33) of the float32
 * result: times 32768, saturated to [-32768, 32767], the fraction dropped toward zero.  Every output is one chain of K fused
 * multiply-adds in fp32, j = 0 .. K - 1 from 0, whatever workgroup computes it: a batch equals its utterances alone and a
 * streamed utterance the whole one, bit for bit.  orig and new must be coprime and at most TTS_RESAMPLE_MAX_FACTOR each
 * (TTS_E_ARG otherwise, the message names the limit). */
int tts_resample(const float* x, const float* table, const TtsResampleSpan* spans, int32_t batch, int64_t max_out_count, int32_t orig,
                 int32_t new_, int32_t w, int32_t pcm16, void* y, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_RESAMPLE_H */
