/*
 * toucan_pitch.h - C ABI of the pitch tracker in libtoucan_hip.so (csrc/pitch.hip): the autocorrelation method of Boersma (1993)
 * with Praat's documented defaults, as the reference's Parselmouth._calculate_f0 asks for it (Preprocessing/PitchCalculator.py:64-67:
 * to_pitch(time_step=256/16000, pitch_floor=40, pitch_ceiling=600)) on the normalised 16 kHz wave.  Written from the published
 * algorithm; PARITY UNPINNED: Praat's own output is not available to compare against (DESIGN.md section 12 holds the definition
 * and tests/pitch_ref.py its float64 restatement).  Same conventions as toucan_align.h: device pointers owned by the caller,
 * ragged packed batches, one hipStream_t per call, 0 or a negative TTS_E_* code, tts_last_error(); an utterance's result depends on
 * that utterance alone.  The only caller is the build's own Python host (ims-toucan-prosody-variance_amd/pitch.py, via ctypes:
 * capi.PITCH_PROTOTYPES).
 */
#ifndef TOUCAN_PITCH_H
#define TOUCAN_PITCH_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_PITCH_CANDIDATES 15        /* per frame: the unvoiced candidate, then at most 14 voiced ones by lag */
#define TTS_PITCH_LAGS 600             /* r[0 .. 599] of a frame */
#define TTS_PITCH_WINDOW 1198          /* samples of the analysis window: 3 periods of 40 Hz */
#define TTS_PITCH_MIN_SAMPLES 1200     /* a shorter wave has no frame */
#define TTS_PITCH_PATH_LDS_FRAMES 2048 /* the most frames whose back-pointers tts_pitch_path keeps in LDS (16 bytes each) */

/* Utterance b is wave[wave_begin[b] ...] (n_samples[b]); its frames are the rows frame_begin[b] ... (n_frames[b]) of the per-frame
 * arrays, with n_frames[b] = (n_samples[b] - 1200) / 256 + 1 and frame f centred between the samples left and left + 1,
 * left = (n_samples[b] - 256 n_frames[b] + 255) / 2 + 256 f (both integer divisions). */

/* stats[2b] = mean of utterance b (summed in fp64 in a fixed order), stats[2b + 1] = max |x - mean|.  One workgroup per utterance. */
int tts_wave_stats(const float* wave, const int32_t* wave_begin, const int32_t* n_samples, int32_t batch, float* stats, tts_stream_t stream);
/* Candidates of every frame, one workgroup per frame (grid max_frames x batch): the mean-free window minus its local mean times
 * win [1198] -> r[k] = ac[k] / (ac[0] wr[k]), k = 0 .. 599 (products and sums in fp32, a fixed order; wr [600] in fp64) -> local
 * maxima above 0.225 among the lags 2 .. 400 -> the best 14 by strength at the parabola's vertex minus the octave cost -> each
 * refined by maximising the windowed sinc interpolation of r (depth 70, fp64).  freq / strength [rows][15]: candidate 0 is the
 * unvoiced one (frequency 0), then the voiced ones by lag, the rest 0; n_cand [rows].  A frame whose utterance's n_frames does not
 * belong to its n_samples gets n_cand -1.  r_out: optional [rows][600], r as fp32. */
int tts_pitch_candidates(const float* wave, const int32_t* wave_begin, const int32_t* n_samples, const float* stats, const int32_t* frame_begin,
                         const int32_t* n_frames, int32_t batch, int32_t max_frames, const float* win, const double* wr, float* freq,
                         float* strength, int32_t* n_cand, float* r_out, tts_stream_t stream);
/* The best path through the candidates (Viterbi, maximising, first maximum on ties; octave, octave-jump and voiced/unvoiced costs
 * of the definition) in fp64, one workgroup per utterance -> f0 [rows]: the chosen frequency, 0 where it is voiceless (0 or above
 * 600 Hz).  Back-pointers, 16 bytes per frame: in LDS (up to lds_frames <= TTS_PITCH_PATH_LDS_FRAMES frames) when
 * scratch_off[b] < 0, else in scratch + scratch_off[b].  An utterance that fits neither, or that has a frame with n_cand outside
 * 1 .. 15, gets f0 -1. */
int tts_pitch_path(const float* freq, const float* strength, const int32_t* n_cand, const int32_t* frame_begin, const int32_t* n_frames,
                   const int64_t* scratch_off, uint8_t* scratch, int32_t batch, int32_t lds_frames, float* f0, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_PITCH_H */
