/*
 * toucan_prominence.h - C ABI of the prominence meter in libtoucan_hip.so (csrc/prominence.hip): which words of an utterance came
 * out prominent in the AUDIO and how strong the breaks between them are, from the continuous wavelet transform of three prosodic
 * tracks (Suni, Simko, Aalto, Vainio, "Hierarchical representation and estimation of prosody using continuous wavelet transform",
 * Computer Speech & Language 45, 2017).  The measure is restated from the publication and simplified where stated below; the
 * authors' toolkit was not at hand, so its parity with that toolkit is NOT pinned - numbers compare only with numbers of this
 * definition.  DESIGN.md section 24 holds the decisions and tests/prominence_ref.py the float64 restatement.  Same conventions as
 * toucan_intelligibility.h: device pointers owned by the caller, one hipStream_t per call, 0 or a negative TTS_E_* code,
 * tts_last_error(); an utterance's result depends on that utterance alone.  The build's own caller is
 * ims-toucan-prosody-variance_amd/prominence.py (ctypes: capi.PROMINENCE_PROTOTYPES).
 *
 * Definition.  An utterance has T frames (1 <= T <= TTS_PROMINENCE_MAX_FRAMES) at one rate for all tracks (the build's front ends
 * run at 62.5 frames/s): f0[t] float32 in Hz, 0 where unvoiced; e[t] float32 > 0, the output of tts_frame_energy; phonemes
 * [begin, end) in frames with a flag "counts for rate"; units [begin, end) to report on (words, or any ranges).  Both tables are
 * ascending and disjoint (begin_k <= end_k <= begin_(k+1)), lie inside [0, T] and may hold empty ranges.
 *
 *   1. Channels, all in fp64.  pitch: ln f0[t], valid where 0 < f0[t] < inf.  energy: ln max(e[t], floor), floor = max(1e-3 max_t e,
 *      2^-126) (the second term only keeps the logarithm of an all-zero track finite), valid everywhere; the comparison is
 *      e[t] > floor ? e[t] : floor, the product 1e-3 (double)max in fp64.  rate: ln(end_k - begin_k) for the frames of phoneme k,
 *      valid where k counts for rate (frames in no phoneme are invalid).
 *   2. Gap filling.  An invalid frame t with the nearest valid frames l < t < r gets v[l] + (v[r] - v[l]) * ((t - l) / (r - l)):
 *      the quotient of the two integers converted to fp64, one product, one sum, nothing contracted.  Before the first valid frame
 *      and after the last the nearest valid value is held; a channel without a valid frame is all 0.
 *   3. z-normalisation over the T frames: mean = sum / T, var = sum of (v - mean)^2 / T, x = (v - mean) / sqrt(var); a channel with
 *      sqrt(var) <= 1e-12 max(1, |mean|) is all 0 (so is every channel of T = 1).  Order of both sums: thread i of 256 adds frames
 *      i, i + 256, .. in ascending order, the 64 lanes of a wavefront are added by the xor butterfly 32, 16, .. 1, the four
 *      wavefronts as ((0 + 1) + 2) + 3.
 *   4. Transform.  psi(u) = 2 / (sqrt(3) pi^(1/4)) (1 - u^2) exp(-u^2 / 2); scales s_j = 2^(j + 1) frames, j = 0 .. 5;
 *      W_c[j][t] = s_j^(-1/2) * sum over k = -8 s_j .. +8 s_j of x_c[t + k] psi(k / s_j), x_c = 0 outside [0, T), k ascending, one
 *      fp64 fused multiply-add per tap from 0, then the one product with s_j^(-1/2): 33, 65, 129, 257, 513 and 1025 taps.  The taps
 *      and the six factors are a table the host builds in float64 (prominence.wavelet_table) - the kernel and the restatement
 *      multiply the same numbers.
 *   5. Composite.  P_c[t] = sum of W_c[j][t] over j = j_lo .. j_hi ascending from 0; P[t] = (w_p P_p[t] + w_e P_e[t]) + w_r P_r[t].
 *      The defaults of the Python layer, weights (1, 1, 0.5) and the band [1, 3] (scales of 4, 8 and 16 frames), are CHOSEN here,
 *      not measured against listeners.
 *   6. Units.  For a unit [b, e) that is not empty: prominence = max of P over it, peak_frame the first frame that attains it,
 *      mean = sum of P / (e - b) (lane l of a wavefront adds frames b + l, b + l + 64, .. ascending, then the xor butterfly), and
 *      pitch_part, energy_part, rate_part = w_c P_c[peak_frame].  An empty unit: NaN and peak_frame -1.
 *   7. Boundaries.  For consecutive non-empty units u < v: boundary_after[u] = -min of P[t] over peak_frame[u] <= t <=
 *      peak_frame[v], valley_frame the first frame that attains the minimum.  The last non-empty unit: NaN and -1.
 *
 * Stated simplification: the publication links the maxima across scales into lines of maximum amplitude and weighs them; here the
 * sum over the band stands in for that, and the linking is not built.  Inputs are taken as finite; a NaN in a track makes the
 * values of its own utterance unspecified and leaves the others alone.
 */
#ifndef TOUCAN_PROMINENCE_H
#define TOUCAN_PROMINENCE_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_PROMINENCE_MAX_FRAMES 65536 /* frames of an utterance: 17.5 minutes at 62.5 frames/s */
#define TTS_PROMINENCE_CHANNELS 3       /* pitch, energy, rate */
#define TTS_PROMINENCE_SCALES 6         /* s_j = 2^(j + 1) */
#define TTS_PROMINENCE_MAX_TAPS 1025    /* 16 s_5 + 1 */
#define TTS_PROMINENCE_TABLE_LD 1026    /* a row of the wavelet table: 1025 taps (zeros past 16 s_j + 1), then s_j^(-1/2) */
#define TTS_PROMINENCE_COLUMNS 8        /* prominence, peak_frame, mean, pitch_part, energy_part, rate_part, boundary_after, valley_frame */
#define TTS_PROMINENCE_UTT_COLUMNS 6    /* a row of the utterance table */
#define TTS_PROMINENCE_TILE 256         /* frames a workgroup of tts_prominence_cwt owns, and a chunk of tts_prominence_channels */

/* The cap on the frames of one utterance: TTS_PROMINENCE_MAX_FRAMES. */
int tts_prominence_max_frames(void);

/* The utterance table, int64 [n_utts][6] on the device and on the host, serves all three entries: (first frame of the utterance in
 * the packed per-frame arrays, T, first row of its phonemes, rows of them, first row of its units, rows of them).  The host rows
 * are checked before a launch - 1 <= T <= the cap, the frames inside total_frames, the rows inside their tables; TTS_E_ARG names
 * the utterance -; a device row that fails the same checks counts as an utterance of no frames.  Utterances must not share frames
 * or rows (not checked).  n_utts: 0 .. 65535.
 *
 * tts_prominence_channels: x (fp64 [3][total_frames]) = the normalised channels (pitch, energy, rate) of every utterance; frames
 * of no utterance are not written.  f0, energy: float32 [total_frames].  phones: int32 [n_phones][3] = (begin, end, counts for
 * rate) in frames of its utterance, on the device and on the host; the host rows are checked (TTS_E_ARG names the utterance and the
 * phoneme), the device rows are only compared with frame numbers, never used as addresses.  One workgroup of 256 per utterance in
 * chunks of 256 frames; the nearest valid frame on either side comes from a backward min-scan and a forward max-scan of frame
 * indices with a carry between the chunks. */
int tts_prominence_channels(const float* f0, const float* energy, int64_t total_frames, const int64_t* utts, const int64_t* utts_host,
                            int32_t n_utts, const int32_t* phones, const int32_t* phones_host, int64_t n_phones, double* x,
                            tts_stream_t stream);

/* w (fp64 [3][6][total_frames]) = W_c[j][t] of every utterance.  table: fp64 [6][1026] on the device (prominence.wavelet_table).
 * A grid of (tiles of 256 frames of the longest utterance, 6, n_utts); a workgroup stages its tile of the three channels with
 * 8 s_j frames on either side (zeros outside the utterance) and the scale's taps in LDS, a thread owns one frame. */
int tts_prominence_cwt(const double* x, int64_t total_frames, const int64_t* utts, const int64_t* utts_host, int32_t n_utts,
                       const double* table, double* w, tts_stream_t stream);

/* rows (fp64 [n_units][8], columns as TTS_PROMINENCE_COLUMNS lists them) for every unit of every utterance; p (fp64
 * [total_frames], or null) = P[t].  units: int32 [n_units][2] = (begin, end) in frames of its utterance, on the device and on the
 * host; the host rows are checked (TTS_E_ARG names the utterance and the unit), a device row is clamped into [0, T].  The weights:
 * finite and >= 0; 0 <= j_lo <= j_hi <= 5.  One workgroup of 256 per utterance, one wavefront per unit. */
int tts_prominence_units(const double* w, int64_t total_frames, const int64_t* utts, const int64_t* utts_host, int32_t n_utts,
                         const int32_t* units, const int32_t* units_host, int64_t n_units, double weight_pitch, double weight_energy,
                         double weight_rate, int32_t j_lo, int32_t j_hi, double* rows, double* p, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_PROMINENCE_H */
