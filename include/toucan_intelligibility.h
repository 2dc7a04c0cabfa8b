/*
 * toucan_intelligibility.h - C ABI of the intelligibility measures in libtoucan_hip.so (csrc/intelligibility.hip): the short-time
 * objective intelligibility of a generated waveform against the recording it is time-aligned with, STOI (Taal, Hendriks, Heusdens,
 * Jensen, IEEE TASL 19(7), 2011), and its extended form ESTOI (Jensen and Taal, IEEE/ACM TASLP 24(11), 2016).  The measure is
 * restated from the two publications; its parity with any toolkit is NOT pinned, and two things are deliberately not copied from
 * any of them: the treatment of the last frame (the compacted signal is framed into exactly M = K frames) and the value of a pair
 * that is too short (NaN, never a sentinel).  DESIGN.md section 23 holds the decisions and tests/intelligibility_ref.py the float64
 * restatement.  Same conventions as toucan_fidelity.h: device pointers owned by the caller, a packed float32 wave, one hipStream_t
 * per call, 0 or a negative TTS_E_* code, tts_last_error(); a pair's result depends on that pair alone.  The build's own caller is
 * ims-toucan-prosody-variance_amd/intelligibility.py (ctypes: capi.INTELLIGIBILITY_PROTOTYPES).
 *
 * Definition.  x is the recording, y the generated signal, both at 10 kHz and n samples long (the host cuts the longer one); eps is
 * the float64 machine epsilon 2^-52.
 *
 *   1. Frames.  Length 256, hop 128, window w[i] = 0.5 (1 - cos(2 pi (i + 1) / 257)), i = 0 .. 255 (the 258-point Hann window
 *      without its zero end points; the kernels are given it as a float32 table, computed in float64 and rounded once).
 *      F = (n - 256) / 128 + 1 frames for n >= 256 (integer division), else none.
 *   2. Silent frames.  e[f] = 20 log10(|| w x_f || + eps) on the recording; frame f is kept iff e[f] > max_f e - 40.  Both signals
 *      keep the same K frames.  Each compacted signal is the overlap-add of its windowed kept frames at hop 128,
 *      128 (K - 1) + 256 samples long.
 *   3. Spectrum.  The compacted signals are framed again (256, hop 128, the same window): M = K frames.  Each frame is zero-padded
 *      to 512 points; bins 0 .. 256 are used.
 *   4. Bands.  15 one-third-octave bands, centres 150 2^(j / 3) Hz, edges 2^(-+1/6) of them, each edge mapped to the nearest of the
 *      257 bin frequencies k 10000 / 512; band j is the bins [edge[j], edge[j + 1]) of TTS_STOI_BAND_EDGES (the upper edge of a
 *      band and the lower edge of the next fall on the same bin).  X_j(m) = sqrt(sum_k |X(k, m)|^2).
 *   5. Segments.  30 consecutive frames: S = M - 29 segments, none for M < 30.  For segment s and band j, x and y are the 30 band
 *      values of the recording and of the generated signal.
 *   6. STOI.  alpha = ||x|| / (||y|| + eps); y' = min(alpha y, (1 + 10^(15/20)) x) element-wise (a NaN on either side is kept);
 *      d = sum (x - mean x)(y' - mean y') / (||x - mean x|| ||y' - mean y'|| + eps).  The segment value is the mean of d over the
 *      15 bands, STOI the mean of the segment values (which is the mean of d over all (j, s)).
 *   7. ESTOI.  The 15 x 30 matrices of a segment: every row has its mean removed and is divided by (its norm + eps), then every
 *      column likewise; d_s = (1 / 30) sum of the element-wise product of the two matrices; ESTOI is the mean of d_s over s.
 *   8. Status (the host's: intelligibility.py).  "too_short": n < 256 or K < 30; both measures are NaN.  Else "ok".  A NaN or Inf
 *      sample makes its pair's measures NaN and leaves the other pairs alone (in the recording it makes the maximum of e NaN or
 *      Inf, no frame passes the comparison, K = 0).
 *
 * Precision and order.  tts_stoi_frame_energy: the products w x in fp32 (one rounding), their squares and the sum in fp64; lane l
 * of a wavefront adds samples l, l + 64, l + 128, l + 192 in this order, the lanes are added by the xor butterfly 32, 16, .. 1.
 * tts_stoi_select: the maximum and the integer scan do not depend on an order.  tts_stoi_gather: compacted sample 128 q + r
 * (r < 128) is fl(fl(0 + fl(w[r + 128] x[128 kept[q - 1] + r + 128])) + fl(w[r] x[128 kept[q] + r])) in fp32, a term whose frame
 * does not exist (q = 0, q = K) counting as +0; a row element is fl(w[i] c) - the materialised overlap-add up to this one addition.
 * The DFT is tts_conv1d (toucan_tts.h, TTS_COMPUTE_F32) with one tap on a [256][2 x 257] basis [cos | -sin].  tts_stoi_bands: the
 * squares (exact) and their sum in fp64, re^2 then im^2 of every bin in ascending order.  tts_stoi_segments: every sum over the 30
 * frames, the 15 bands or the 30 columns is one chain in ascending order, all in fp64.  tts_stoi_reduce: thread t of 256 adds
 * segments t, t + 256, .. in ascending order, then the xor butterfly, then the four wavefronts as ((0 + 1) + 2) + 3.  None depends
 * on what else is in the batch: a batch equals its pairs alone bit for bit.
 */
#ifndef TOUCAN_INTELLIGIBILITY_H
#define TOUCAN_INTELLIGIBILITY_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_STOI_RATE 10000
#define TTS_STOI_FRAME 256
#define TTS_STOI_HOP 128
#define TTS_STOI_BINS 257
#define TTS_STOI_BANDS 15
#define TTS_STOI_SEGMENT 30
#define TTS_STOI_MAX_FRAMES 8388608 /* 2^23 frames of a pair: 29 hours */
/* band j = bins [edge[j], edge[j + 1]) */
#define TTS_STOI_BAND_EDGES 7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219

/* Frames one sweep of tts_stoi_select covers, and segments one workgroup of tts_stoi_segments owns. */
int tts_stoi_select_sweep(void);
int tts_stoi_segments_per_group(void);

/* pairs: int64 [n_pairs][3] = (first sample of the recording, first sample of the generated signal, samples n of both) into the
 * packed wave x (float32 [n_samples]), on the device and on the host.  The host rows are checked before a launch (both signals
 * inside the wave, F <= max_frames; TTS_E_ARG names the pair); a device row that fails the same checks counts as a pair of no
 * frames.  max_frames: 1 .. TTS_STOI_MAX_FRAMES, at least the frames of the longest pair.  window: float32 [256] on the device.
 *
 * energy[p][f] (fp64 [n_pairs][max_frames]) = || w x_f ||^2 of the recording of pair p for f < F_p; the other slots are not
 * written.  A grid of (groups of 4 frames of the longest pair, n_pairs), one wavefront per frame. */
int tts_stoi_frame_energy(const float* x, int64_t n_samples, const int64_t* pairs, const int64_t* pairs_host, int32_t n_pairs,
                          const float* window, int64_t max_frames, double* energy, tts_stream_t stream);

/* kept[p][0 .. K_p - 1] (int32 [n_pairs][max_frames]) = the frames with e[f] > max e - 40 in ascending order, counts[p] = K_p
 * (int32 [n_pairs]); the slots past K_p are not written.  One workgroup per pair in sweeps of tts_stoi_select_sweep() frames. */
int tts_stoi_select(const double* energy, const int64_t* pairs, const int64_t* pairs_host, int32_t n_pairs, int64_t n_samples,
                    int64_t max_frames, int32_t* kept, int32_t* counts, tts_stream_t stream);

/* The windowed frames of the compacted signals, never materialised: rows (float32 [total_rows][256]) gets, from row
 * row_begin[p][0] for the recording and row_begin[p][1] for the generated signal (int64 [n_pairs][2] on the device and on the
 * host; F_p rows each, inside total_rows - checked on the host rows -, not overlapping - not checked), row m < K_p = frame m of the
 * compacted signal and rows K_p .. F_p - 1 = zeros.  kept and counts: what tts_stoi_select left (an index outside 0 .. F_p - 1 is
 * clamped into it, a count outside 0 .. F_p counts as 0).  A grid of (groups of 4 rows, n_pairs, 2); a thread stores 16 bytes. */
int tts_stoi_gather(const float* x, int64_t n_samples, const int64_t* pairs, const int64_t* pairs_host, int32_t n_pairs,
                    const float* window, int64_t max_frames, const int32_t* kept, const int32_t* counts, const int64_t* row_begin,
                    const int64_t* row_begin_host, int64_t total_rows, float* rows, tts_stream_t stream);

/* bands[r][j] (fp64 [total_rows][15]) of every row of spec (float32 [total_rows][ld], row = [re(0 .. 256) | im(0 .. 256)],
 * ld >= 514). */
int tts_stoi_bands(const float* spec, int64_t ld, int64_t total_rows, double* bands, tts_stream_t stream);

/* segments[p][s][0 .. 1] (fp64 [n_pairs][max_segments][2], max_segments = max(1, max_frames - 29)) = the STOI and ESTOI value of
 * segment s < S_p = K_p - 29 of pair p; the other slots are not written.  bands: fp64 [total_rows][15]; row_begin as for
 * tts_stoi_gather; frames: int64 [n_pairs] on the host, F_p (checked against max_frames and total_rows; the device reads counts
 * alone and takes a count outside 0 .. max_frames or past total_rows as 0).  A grid of (groups of tts_stoi_segments_per_group()
 * segments of the longest pair, n_pairs); a workgroup stages its group's frames of both band arrays in LDS once. */
int tts_stoi_segments(const double* bands, int64_t total_rows, const int64_t* row_begin, const int64_t* row_begin_host,
                      const int64_t* frames_host, const int32_t* counts, int32_t n_pairs, int64_t max_frames, double* segments,
                      tts_stream_t stream);

/* totals[p][0 .. 1] (fp64 [n_pairs][2]) = STOI and ESTOI of pair p, the means over its S_p segments; NaN for a pair of none. */
int tts_stoi_reduce(const double* segments, const int32_t* counts, int32_t n_pairs, int64_t max_frames, double* totals,
                    tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_INTELLIGIBILITY_H */
