/*
 * toucan_prosody_fit.h - C ABI of the time-budget solver in libtoucan_hip.so (kernels: csrc/prosody.hip; stage entry:
 * csrc/pipeline.hip).  toucan_prosody.h and toucan_prosody_curves.h scale durations relatively; here an utterance, its pauses or a
 * span of its phonemes is fitted to an absolute number of mel frames, on the device, between the predictors and the control kernel
 * of the same pass.
 *
 * A SEGMENT is a packed row range [begin, end) of one utterance with a target T in mel frames (an integer, 1 <= T <= 2^24), a knob
 * and bounds lo <= hi (finite, hi <= 64).  Its kind names the knob:
 *     0 UTT_DURATION  the whole utterance; the knob is the utterance's duration scale S.duration; lo > 0  (defaults 0.25 .. 4)
 *     1 UTT_PAUSE     the whole utterance; the knob is its pause scale S.pause;                   lo >= 0 (defaults 0 .. 8)
 *     2 SPAN          a row range; the knob is a multiplier m; row r of the span gets curve column 0
 *                     c'_r = fl(c_r * m), c_r = 1 without a curve table;                          lo > 0  (defaults 0.25 .. 4)
 *
 * F(x) is the number of frames tts_prosody_control_v / _c will produce for the segment's rows with the knob at x and everything else
 * as given: per row, with the duration d after the overrides (0 at a word boundary),
 *     d'  = (silence && pause != 1) ? (int)rintf((float)d * pause) : d
 *     ed  = S.duration * c                              (one fp32 product)
 *     d'' = ed != 1 ? (int)rintf((float)d' * ed) : d'
 * - one __device__ function that the control kernel and the solver both call - summed in 64-bit integers.  F does not decrease in x.
 *
 * Non-negative fp32 values are ordered by their bit patterns.  The solve:
 *     F(lo) == F(hi)   EMPTY         the knob keeps its given value, nothing is written for the segment
 *     F(lo) >  T       CLAMPED_LOW   knob = lo
 *     F(hi) <  T       CLAMPED_HIGH  knob = hi
 *     else bisect on the bit pattern for the smallest x1 in (lo, hi] with F(x1) >= T (at most 31 steps; x1 = lo if F(lo) >= T
 *     already); x0 is the fp32 predecessor of x1.
 *         F(x1) == T          EXACT     knob = x1
 *         else, exact != 0    REPAIRED  knob = x0, and the k = T - F(x0) missing frames go to the rows that change between x0 and x1:
 *                                       delta_r = d''_r(x1) - d''_r(x0) >= 0, n = sum of delta_r >= k; row r owns the slots
 *                                       [p_r, p_r + delta_r) of the exclusive prefix sum p in row order; slot t is taken when
 *                                       floor((t + 1) k / n) > floor(t k / n) (64-bit integers: exactly k slots, evenly spread);
 *                                       extra_r = the taken slots that row r owns
 *         else                NEAREST   knob = whichever of x0, x1 has the smaller |F - T|, x0 on a tie; every extra is 0
 *
 * Outputs: scales_out [n_seq][4], the input table (or all ones) with the solved knobs of the kinds 0 and 1 written in; curves_out
 * [rows][5], the input table (or neutral rows 1 1 1 0 0) with column 0 of the rows of solved SPAN segments rewritten; extra, int32
 * [rows], zero outside REPAIRED segments; report [n_seg][8] with the columns
 *     0 target   1 frames (F(value) + the segment's extra)   2 frames_scaled (F(value))   3 value   4 status   5 iterations
 *     6 extra_rows (rows with extra > 0)   7 base_frames (F at the knob's given value: what the call would have produced)
 * every entry below 2^24 and therefore exact in fp32.  tts_prosody_control_v / _c with the written tables, then
 * tts_prosody_fit_apply, give an EXACT or REPAIRED segment exactly T frames.
 * Same conventions as toucan_prosody.h; the build's own callers are engine.py and native.py (ctypes: capi.FIT_PROTOTYPES).
 * DESIGN.md section 22 holds the decisions and tests/prosody_fit_ref.py the numpy restatement.
 */
#ifndef TOUCAN_PROSODY_FIT_H
#define TOUCAN_PROSODY_FIT_H

#include "toucan_prosody_curves.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_FIT_UTT_DURATION 0
#define TTS_FIT_UTT_PAUSE 1
#define TTS_FIT_SPAN 2

#define TTS_FIT_EMPTY 0
#define TTS_FIT_EXACT 1
#define TTS_FIT_REPAIRED 2
#define TTS_FIT_NEAREST 3
#define TTS_FIT_CLAMPED_LOW 4
#define TTS_FIT_CLAMPED_HIGH 5

#define TTS_FIT_SPEC 4     /* floats per segment of seg_spec: target, lo, hi, exact (0 or 1) */
#define TTS_FIT_COLUMNS 8  /* floats per segment of the report, and of the stage entry's host segment table */
#define TTS_FIT_MAX_TARGET 16777216 /* 2^24 */
#define TTS_FIT_MAX_BOUND 64

/* The solve above, one workgroup per segment; a segment's result depends on that segment alone.  All pointers are device pointers.
 * text / dur / seq_begin / seq_end as for tts_prosody_control_v (dur is read, not written).  seg_begin / seg_end: packed row
 * ranges; seg_seq: the utterance of each; seg_kind: TTS_FIT_*; seg_spec [n_seg][4].  scales_in [n_seq][4] or NULL (all 1);
 * curves_in [rows][5] or NULL.  curves_out may be NULL when curves_in is NULL and no segment is a SPAN.  Before the solve, on the
 * same stream, scales_out and the utterances' rows of curves_out are filled from the inputs (or with neutral values) and the
 * utterances' rows of extra are zeroed; rows that no utterance covers are not touched.  Segments of one utterance must be disjoint
 * and an utterance has either one UTT_* segment or SPAN segments; the specs must satisfy the limits above: the caller checks that
 * (tts_control_and_regulate_t does), the kernel does not.  TTS_E_ARG for a negative count, a null pointer, ld_text < 62. */
int tts_prosody_fit(const float* text, int32_t ld_text, const int32_t* dur, const int32_t* seq_begin, const int32_t* seq_end, int32_t n_seq,
                    const int32_t* seg_begin, const int32_t* seg_end, const int32_t* seg_seq, const int32_t* seg_kind, int32_t n_seg,
                    const float* seg_spec, const float* scales_in, const float* curves_in, float* scales_out, float* curves_out,
                    int32_t* extra, float* report, tts_stream_t stream);

/* dur[r] += extra[r] for r < rows: after the control kernel, the frames the repair hands out. */
int tts_prosody_fit_apply(int32_t* dur, const int32_t* extra, int32_t rows, tts_stream_t stream);

/* Stage entry: tts_control_and_regulate_c with a segment table (host, [n_seg][8], n_seg >= 1; columns: utterance, kind, begin, end
 * (packed rows), target, lo, hi, exact).  scales (host [B][4]), curves (host [R][5]) and spans (host [n_spans][2], with curves only)
 * may be NULL.  Runs overrides -> statistics -> tts_prosody_fit -> tts_prosody_control_v / _c with the written tables ->
 * tts_prosody_fit_apply -> statistics -> the duration read-back and the length regulator: the statistics "after" include the extra
 * frames.  The writable tables, extra and the report live in the handle's workspace; the caller's tables in the table store are
 * read only.  The report, the solved scales and extra come back in front of the durations, in the entry's one host
 * synchronisation.  Everything is checked on the host before anything is enqueued (TTS_E_ARG; the message names the utterance and
 * the segment): kinds, ranges inside their utterance and not empty, a UTT_* segment covers its whole utterance and is alone in it,
 * SPAN segments of an utterance do not overlap, targets, bounds, and what tts_control_and_regulate_c checks. */
int tts_control_and_regulate_t(TtsHandle* h, const float* scales, const float* curves, const int32_t* spans, int32_t n_spans,
                               const float* segments, int32_t n_seg, int32_t* frame_counts, tts_stream_t stream);

/* What the last tts_control_and_regulate_t of the batch in flight left in the handle -> report (host [n_seg][8]), scales (host
 * [B][4], the solved table) and extra (host int32 [R]); each may be NULL.  A host copy: nothing is enqueued on `stream`.  TTS_E_ARG
 * if the batch in flight did not go through tts_control_and_regulate_t. */
int tts_copy_prosody_fit(TtsHandle* h, float* report, float* scales, int32_t* extra, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_PROSODY_FIT_H */
