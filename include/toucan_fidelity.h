/*
 * toucan_fidelity.h - C ABI of the spectral distances in libtoucan_hip.so (csrc/fidelity.hip): how far a generated 24 kHz waveform
 * is from the recording it was generated from, in the unit the reference trains its vocoders in (MelSpectrogramLoss.py: the L1
 * distance of log10 mel amplitudes) and as multi-resolution STFT distances.  DESIGN.md section 21 holds the decisions and
 * tests/fidelity_ref.py the float64 restatement.  Same conventions as toucan_truepeak.h: device pointers owned by the caller, a
 * packed float32 wave with one (begin, count) span per utterance on the device and on the host, one hipStream_t per call, 0 or a
 * negative TTS_E_* code, tts_last_error(); an utterance's (a pair's) result depends on that utterance (pair) alone.  The build's
 * own caller is ims-toucan-prosody-variance_amd/fidelity.py (ctypes: capi.FIDELITY_PROTOTYPES).
 *
 * Definition.  a is the generated signal, b the recording, both n samples long (the host cuts the longer one).  A resolution is
 * (N, hop = N / 4) and, for the reference resolution (1536, 384) only, a mel filterbank.
 *
 *   Framing.  The signal is padded by reflection with N / 2 samples on both sides, p[j] = x[N / 2 - j] in front and
 *   p[N / 2 + n + k] = x[n - 2 - k] behind (numpy.pad(mode="reflect"): the edge sample is not repeated), which needs n > N / 2.
 *   Frame f covers p[f hop .. f hop + N), f = 0 .. F - 1, F = 1 + n / hop (integer division): torch.stft(center=True).  The
 *   window is the periodic Hann, w[i] = 0.5 - 0.5 cos(2 pi i / N).  With p viewed as rows of hop samples, a frame is four
 *   consecutive rows: the DFT is tts_conv1d (toucan_tts.h, TTS_COMPUTE_F32: exact fp32 products, fp32 accumulation) with 4 taps
 *   on a [4][hop][2 (N / 2 + 1)] basis, columns [w cos | -w sin], which leaves row f = [re(0 .. N / 2) | im(0 .. N / 2)].
 *   Amplitude.  amp[k] = sqrt(max(re^2 + im^2, 1e-10)), in fp32: fl(fma(im, im, fl(re re))), the clamp, the correctly rounded root.
 *   mel_l1.  e[m] = sum_k M[m][k] amp[k]; the term of (frame, band) is | log10 max(e_a, 1e-10) - log10 max(e_b, 1e-10) | and
 *   mel_l1 the mean of the terms over F x n_mels.  M is the Slaney filterbank of librosa.filters.mel(24000, 1536, 100, 80, 12000)
 *   (style.mel_filterbank): every band is one run of 4 to 50 consecutive bins, so it is given as runs - (first, count) per band
 *   and the non-zero weights of all bands one after the other.  e[m] is one chain of fp32 fused multiply-adds in ascending k from
 *   0; the two log10 and everything after them are fp64.
 *   spectral_convergence = sqrt(sum (amp_a - amp_b)^2) / sqrt(sum amp_b^2) over all frames and bins (the differences and squares
 *   in fp64); the clamp of the amplitude keeps the denominator positive for silence.
 *   log_magnitude_l1 = the mean over F x (N / 2 + 1) of | ln amp_a - ln amp_b |, the logarithms in fp64 of the fp32 amplitudes.
 *   frame_mel_l1[f] = the mean of frame f's mel terms over n_mels.
 *   A clamp is `v < floor ? floor : v`: a NaN stays a NaN and ends in the sums of its own frame, hence of its own pair, only.
 *
 * Order of the sums.  tts_spectral_distance: thread t of the 256 of a workgroup adds the terms of bins t, t + 256, ... in
 * ascending order (for the mel term: thread m holds band m); the 64 lanes of a wavefront are added by the xor butterfly 32, 16,
 * .. 1, and the four wavefronts as ((0 + 1) + 2) + 3.  tts_spectral_reduce: thread t adds frames t, t + 256, ... in ascending
 * order, then the same butterfly.  Neither depends on what else is in the batch: a batch equals its pairs alone bit for bit.
 */
#ifndef TOUCAN_FIDELITY_H
#define TOUCAN_FIDELITY_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_FIDELITY_SUMS 4         /* per frame and per pair: sum |d log10 mel|, sum (d amp)^2, sum amp_b^2, sum |d ln amp| */
#define TTS_FIDELITY_MAX_BINS 2049  /* N / 2 + 1 up to N = 4096: two amplitude rows of a frame in LDS */
#define TTS_FIDELITY_MAX_BANDS 256  /* one thread per mel band */
#define TTS_FIDELITY_MAX_HOP 4096

/* Frames of a pair one workgroup of tts_spectral_distance takes, and frames one sweep of tts_spectral_reduce covers. */
int tts_spectral_frames_per_group(void);
int tts_spectral_reduce_sweep(void);

/* The padded row buffer of a ragged batch: utterance u (spans as in toucan_loudness.h: int64 [batch][2] = (first sample, sample
 * count) on the device and on the host) with n samples becomes R = 4 + ceil(n / hop) rows of `hop` floats from row row_begin[u]
 * of `rows` (float32 [total_rows][hop]): 2 hop reflected samples, the n samples, 2 hop reflected samples, zeros to the end of the
 * last row.  This is the buffer align.batched_spectra builds on the host (at hop 256 byte for byte).  row_begin: int64 [batch] on
 * the device and on the host; the host rows are checked before the launch: every n > 2 hop (TTS_E_ARG names the utterance),
 * row_begin[u] >= 0 and row_begin[u] + R <= total_rows; a device row that fails the same checks is skipped.  The row ranges of
 * different utterances must not overlap (not checked).  hop: a multiple of 4 up to TTS_FIDELITY_MAX_HOP.  max_count >= every n.
 * One launch: a grid of (tiles of the longest utterance's rows, batch), 4 consecutive outputs per thread, one 16-byte store. */
int tts_frame_reflect(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, int64_t max_count,
                      int32_t hop, const int64_t* row_begin, const int64_t* row_begin_host, int64_t total_rows, float* rows,
                      tts_stream_t stream);

/* frame_sums[p][f][0 .. 3] (fp64 [n_pairs][max_frames][TTS_FIDELITY_SUMS]) for f = 0 .. frames_p - 1 of every pair; the other
 * slots are not written.  spec: float32 [total_rows][ld], row r = [re(0 .. bins - 1) | im(0 .. bins - 1)], ld >= 2 bins.  pairs:
 * int64 [n_pairs][3] = (first row of a's frames, first row of b's frames, frames) on the device and on the host; the host rows
 * are checked (rows inside spec, frames <= max_frames; TTS_E_ARG names the pair), a device row that fails counts as 0 frames.
 * bands: int32 [n_bands][2] = (first bin, count) on the device and on the host, weights: float32 [n_weights] on the device, the
 * runs one after the other (n_weights = the sum of the counts, checked on the host rows, as is first + count <= bins);
 * n_bands = 0 (bands, weights NULL): no filterbank, sum 0 is written as 0.  A grid of (groups of tts_spectral_frames_per_group()
 * frames of the longest pair, n_pairs); per frame the two amplitude rows go to LDS once and nothing but the four sums leaves. */
int tts_spectral_distance(const float* spec, int64_t ld, int32_t bins, int64_t total_rows, const int64_t* pairs, const int64_t* pairs_host,
                          int32_t n_pairs, int64_t max_frames, const int32_t* bands, const int32_t* bands_host, int32_t n_bands,
                          const float* weights, int32_t n_weights, double* frame_sums, tts_stream_t stream);

/* totals[p][0 .. 3] (fp64 [n_pairs][TTS_FIDELITY_SUMS]) = the sums over the frames of pair p, one workgroup per pair; 0 for a
 * pair of no frames.  pairs: as above (column 2 is read; a value outside 0 .. max_frames counts as 0). */
int tts_spectral_reduce(const double* frame_sums, const int64_t* pairs, int32_t n_pairs, int64_t max_frames, double* totals,
                        tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_FIDELITY_H */
