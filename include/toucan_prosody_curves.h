/*
 * toucan_prosody_curves.h - C ABI of the per-phoneme prosody curves in libtoucan_hip.so (kernel: csrc/prosody.hip, the one the
 * other two control entries launch; stage entries: csrc/pipeline.hip).  toucan_prosody.h gives every utterance of a ragged batch its own four scales; here every PHONEME has
 * its own: a curve table, float32 [rows][5] over the packed phoneme rows, whose columns are
 *
 *     0 duration factor   1 pitch variance scale   2 energy variance scale   (neutral 1)      3 pitch offset   4 energy offset   (neutral 0)
 *
 * With S the utterance's four scales (all 1 when there are none) and C[r] row r of the table, one workgroup per utterance computes:
 *   1. the linguistic overrides of tts_prosody_control_v (pitch 0 where unvoiced, energy 0 off phonemes, duration 0 at word
 *      boundaries), the pause scale on silence rows where it is not 1, then ed = S.duration * C[r][0] (one fp32 product) and, where
 *      ed != 1, d = (int)rintf((float)d * ed);
 *   2. for pitch, and likewise energy: avg = the mean over the non-zero entries of the WHOLE utterance (always computed); per row
 *      es = S.pitch * C[r][1] (one fp32 product); where es != 1 the row becomes max(0, (v - avg) * es + avg), where es == 1 the row is
 *      not written - (v - avg) * 1 + avg is not v in fp32;
 *   3. with o = C[r][3] (C[r][4]): where o != 0 and the row's value after step 2 is not 0, v = max(0, v + o).  Unvoiced rows stay
 *      unvoiced and rows off phonemes keep energy 0.
 * An all-neutral table gives the bits of tts_prosody_control_v with S; a table constant over an utterance at (c_d, c_p, c_e, 0, 0) with
 * S = 1 gives the bits of the scalar tts_prosody_control with those three values (1 * c == c), the NaN mean of an utterance without a
 * non-zero entry included; a row that is neutral under S = 1 keeps its bits whatever other rows do.  The reference's _scale_variance
 * shifts zeros too: a zero inside a span scaled below 1 becomes avg * (1 - es), here as there.
 *
 * Statistics of a span need no entry of their own: tts_prosody_stats (toucan_prosody.h) takes arbitrary [begin, end) row ranges, so
 * a span of phonemes is one more "sequence" of its call.  Column 6 of a span's block is then the frames the span occupies.
 * Same conventions as toucan_prosody.h; the build's own callers are engine.py and native.py (ctypes: capi.CURVE_PROTOTYPES).
 * DESIGN.md section 15 holds the definition and tests/prosody_curves_ref.py its float64 restatement.
 */
#ifndef TOUCAN_PROSODY_CURVES_H
#define TOUCAN_PROSODY_CURVES_H

#include "toucan_prosody.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_PROSODY_CURVE_COLUMNS 5 /* floats per phoneme row: duration factor, pitch variance scale, energy variance scale, pitch offset, energy offset */

/* The definition above on a packed ragged batch.  scales: device [n_seq][4] in toucan_prosody.h's order, or NULL for all 1; curves:
 * device [rows][5] indexed by packed row (the rows no utterance covers are not read).  Nothing is validated here: a duration factor
 * must be positive and finite and the other columns finite, which the stage entry checks on its host values. */
int tts_prosody_control_c(const float* text, int32_t ld_text, float* pitch, float* energy, int32_t* dur, const int32_t* seq_begin,
                          const int32_t* seq_end, int32_t n_seq, const float* scales, const float* curves, tts_stream_t stream);

/* Stage entry: tts_control_and_regulate_v with a curve table (host, [R][5], R the batch's phoneme rows) and optional spans (host,
 * [n_spans][2] packed row ranges [begin, end) with 0 <= begin <= end <= R, at most R of them; NULL with n_spans 0).  scales: host
 * [B][4] or NULL.  Runs overrides -> statistics over utterances and over spans -> tts_prosody_control_c -> both statistics again ->
 * the duration read-back and the length regulator.  The table and the span bounds go to the device through the handle's pinned
 * table staging, one asynchronous copy each on `stream`; the statistics come back in front of the durations, in the entry's one host
 * synchronisation.  TTS_E_ARG for a duration factor that is not positive and finite, another column that is not finite (the message
 * names the utterance and the phoneme) and a span outside the batch; nothing is enqueued then.  tts_copy_prosody_stats returns the
 * utterance blocks afterwards as after tts_control_and_regulate_v. */
int tts_control_and_regulate_c(TtsHandle* h, const float* scales, const float* curves, const int32_t* spans, int32_t n_spans,
                               int32_t* frame_counts, tts_stream_t stream);

/* The span blocks the last tts_control_and_regulate_c of the batch in flight left in the handle -> before / after (host,
 * [n_spans][8] each, columns as TTS_PROSODY_STATS; either may be NULL).  A host copy: nothing is enqueued on `stream`.  TTS_E_ARG if
 * the batch in flight did not go through tts_control_and_regulate_c. */
int tts_copy_prosody_span_stats(TtsHandle* h, float* before, float* after, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_PROSODY_CURVES_H */
