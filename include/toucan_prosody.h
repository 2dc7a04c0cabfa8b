/*
 * toucan_prosody.h - C ABI of the per-utterance prosody scales in libtoucan_hip.so (kernels: csrc/prosody.hip, stage entries:
 * csrc/pipeline.hip).  The four knobs of the reference's inference call - duration_scaling_factor, pitch_variance_scale,
 * energy_variance_scale, pause_duration_scaling_factor (InferenceToucanTTS.py:214-227 + _scale_variance :333-343) - are scalars of a
 * whole batch in toucan_tts.h (tts_prosody_control, tts_control_and_regulate).  Here every utterance of a ragged batch has its own
 * four, and the statistics of its pitch, energy and durations can be taken before and after the scales were applied: the
 * reference's _scale_variance shifts the zeros too and clamps negatives to 0, so a requested variance scale is not the realised one.
 * Same conventions as toucan_pitch.h: device pointers owned by the caller, ragged packed batches, one hipStream_t per call, 0 or a
 * negative TTS_E_* code, tts_last_error(); an utterance's result depends on that utterance alone.  The build's own callers are
 * ims-toucan-prosody-variance_amd/engine.py and native.py (ctypes: capi.PROSODY_PROTOTYPES).  DESIGN.md section 14 holds the definition
 * and tests/prosody_ref.py its float64 restatement.
 */
#ifndef TOUCAN_PROSODY_H
#define TOUCAN_PROSODY_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_PROSODY_SCALES 4 /* floats per utterance: duration, pitch variance, energy variance, pause duration */
#define TTS_PROSODY_STATS 8  /* floats per utterance: n_pitch, mean_pitch, var_pitch, n_energy, mean_energy, var_energy, frames, phones */

/* tts_prosody_control with the four scales of utterance u read from scales[4 u ...] (device, [n_seq][4]); one workgroup per
 * utterance.  A scale that is exactly 1.0f skips its step for that utterance, as the scalar kernel does for the batch - (v - avg) * 1
 * + avg is not v in fp32 - and the order of operations and of the reductions is the scalar kernel's: utterance u comes out
 * bit-identical to tts_prosody_control run on it alone with its own four scalars, the NaN mean of an utterance without a non-zero
 * entry whose variance scale is not 1 included.  scales == NULL: the linguistic overrides alone (pitch 0 where unvoiced, energy 0
 * off phonemes, duration 0 at word boundaries) and no scale; a call with scales after one without gives the bits of the one call
 * with scales (the overrides are idempotent).  The scales are not validated here: a duration scale must be positive and finite,
 * which the stage entry checks on its host values. */
int tts_prosody_control_v(const float* text, int32_t ld_text, float* pitch, float* energy, int32_t* dur, const int32_t* seq_begin,
                          const int32_t* seq_end, int32_t n_seq, const float* scales, tts_stream_t stream);

/* stats[8 u ...] (device, [n_seq][8]) of utterance u = {n_pitch, mean_pitch, var_pitch, n_energy, mean_energy, var_energy, frames,
 * phones}: n_* counts the non-zero entries, mean and population variance are taken over those alone (both 0 when there is none),
 * frames is the sum of the durations, phones the rows.  Two passes - the mean, then the squared deviations from it - accumulated in
 * fp64 in a fixed order (thread t takes rows t, t + 256, ...; lanes, then wavefronts are folded in one fixed tree) and rounded to
 * fp32 once at the store: a row of the result does not depend on the batch the utterance is in.  One workgroup per utterance. */
int tts_prosody_stats(const float* pitch, const float* energy, const int32_t* dur, const int32_t* seq_begin, const int32_t* seq_end,
                      int32_t n_seq, float* stats, tts_stream_t stream);

/* Stage entry: tts_control_and_regulate with per-utterance scales (host, [B][4] in the order above).  Runs overrides -> statistics
 * -> scales -> statistics -> the duration read-back and the length regulator of tts_control_and_regulate, and leaves both
 * statistics blocks in the handle.  The scales go to the device through the handle's pinned table staging on `stream`; the
 * statistics come back with the durations, in the one host round trip the scalar entry already has - no other synchronisation.
 * A duration scale that is not positive and finite is TTS_E_ARG, the message names the utterance; nothing is enqueued then. */
int tts_control_and_regulate_v(TtsHandle* h, const float* scales, int32_t* frame_counts, tts_stream_t stream);

/* The statistics the last tts_control_and_regulate_v of the batch in flight left in the handle -> before / after (host, [B][8] each;
 * either may be NULL): before = after the overrides and before the scales, after = after the scales.  They were read back inside
 * tts_control_and_regulate_v, so this is a host copy: nothing is enqueued on `stream`.  TTS_E_ARG if the batch in flight went
 * through the scalar tts_control_and_regulate. */
int tts_copy_prosody_stats(TtsHandle* h, float* before, float* after, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_PROSODY_H */
