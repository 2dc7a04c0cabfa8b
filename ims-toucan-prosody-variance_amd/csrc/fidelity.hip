// Spectral distances between a generated waveform and its recording (include/toucan_fidelity.h):
//   tts_frame_reflect      packed waves -> the reflection-padded row buffer [rows, hop] a 4-tap conv turns into the STFT
//   tts_spectral_distance  the two spectra of every pair -> four fp64 sums per frame (log-mel L1, the two parts of the spectral
//                          convergence, log-magnitude L1); amplitudes, mel energies and logarithms stay on the chip
//   tts_spectral_reduce    the per-frame sums of every pair -> [pairs, 4]
// The DFT between the first two is tts_conv1d in fp32 (conv1d.hip).  Every sum runs in a fixed order that does not depend on the
// batch; there are no atomics.
#include <math.h>

#include "segment_scan.h"
#include "../../include/toucan_fidelity.h"

namespace tts {

constexpr int FD_THREADS = 256;
constexpr int FR_PER_THREAD = 4;                       // outputs per thread of frame_reflect_kernel: one 16-byte store
constexpr int FR_TILE = FD_THREADS * FR_PER_THREAD;
constexpr int SD_FRAMES = 4;                           // frames per workgroup of spectral_distance_kernel
constexpr int SD_MAX_WEIGHTS = 4096;                   // filterbank weights kept in LDS (the reference resolution has 1.6 k)
constexpr int NS = TTS_FIDELITY_SUMS;

// rows of the padded buffer of an utterance of n samples: 2 hop + n + 2 hop samples, rounded up to whole rows
__host__ __device__ __forceinline__ int64_t padded_rows(int64_t n, int hop) { return 4 + (n + hop - 1) / hop; }

__global__ __launch_bounds__(FD_THREADS) void frame_reflect_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                                   int hop, const int64_t* __restrict__ row_begin, int64_t total_rows,
                                                                   float* __restrict__ rows) {
  const int u = blockIdx.y;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t n = sp.count, pad = 2 * (int64_t)hop;
  if (n <= pad) return;  // (also a span outside the wave: count 0) - the reflection would leave the utterance
  const int64_t R = padded_rows(n, hop), rb = row_begin[u];
  if (rb < 0 || R > total_rows || rb > total_rows - R) return;
  const int64_t j0 = ((int64_t)blockIdx.x * FD_THREADS + threadIdx.x) * FR_PER_THREAD;
  if (j0 >= R * hop) return;  // hop is a multiple of 4: a thread's four outputs are inside the buffer or all outside
  const float* __restrict__ src = x + sp.begin;
  f32x4 v;
#pragma unroll
  for (int e = 0; e < FR_PER_THREAD; ++e) {
    const int64_t j = j0 + e;
    float s = 0.0f;                                   // the tail of the last row
    if (j < pad) s = src[pad - j];                    // 1 <= pad - j <= pad <= n - 1
    else if (j < pad + n) s = src[j - pad];
    else if (j < n + 2 * pad) s = src[2 * n + pad - 2 - j];  // n - 2 - (j - pad - n): from n - 2 down to n - 1 - pad >= 0
    v[e] = s;
  }
  *reinterpret_cast<f32x4*>(rows + rb * hop + j0) = v;  // (rb hop + j0) is a multiple of 4 and `rows` 16-byte aligned
}

struct PairRows {
  int64_t a, b, frames;
};

// a row that does not lie inside the spectrum counts as a pair of no frames
__device__ __forceinline__ PairRows load_pair(const int64_t* __restrict__ pairs, int p, int64_t total_rows, int64_t max_frames) {
  PairRows r = {pairs[3 * p], pairs[3 * p + 1], pairs[3 * p + 2]};
  if (r.frames < 0 || r.frames > max_frames || r.frames > total_rows || r.a < 0 || r.b < 0 || r.a > total_rows - r.frames ||
      r.b > total_rows - r.frames)
    r.frames = 0;
  return r;
}

// sqrt(max(re^2 + im^2, 1e-10)); a NaN passes the clamp
__device__ __forceinline__ float amplitude(float re, float im) {
  const float p = __builtin_fmaf(im, im, __fmul_rn(re, re));
  return __fsqrt_rn(p < 1e-10f ? 1e-10f : p);
}

// The NS sums of the workgroup in the butterfly order of wave_ops.h, left in red[q][wavefront]; thread 0 folds the wavefronts
// (fold_sums) after the ONE barrier this returns behind: the wavefront layer and not block_sum, whose barrier before the write
// the callers' own barriers stand in for (see there).  Every thread calls it.
__device__ __forceinline__ void wave_partials(double (&s)[NS], double (*red)[4]) {
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    s[q] = wave_sum(s[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = s[q];
  }
  __syncthreads();
}

__device__ __forceinline__ double fold_sums(const double* red) {
  return fold_left(red, [](double a, double b) { return a + b; });
}

__global__ __launch_bounds__(FD_THREADS) void spectral_distance_kernel(const float* __restrict__ spec, int64_t ld, int bins, int64_t total_rows,
                                                                       const int64_t* __restrict__ pairs, int64_t max_frames,
                                                                       const int* __restrict__ bands, int n_bands,
                                                                       const float* __restrict__ weights, int n_weights,
                                                                       double* __restrict__ frame_sums) {
  __shared__ float amp[2][TTS_FIDELITY_MAX_BINS];
  __shared__ float wts[SD_MAX_WEIGHTS];
  __shared__ int counts[TTS_FIDELITY_MAX_BANDS];
  __shared__ double red[NS][4];
  const int p = blockIdx.y, tid = threadIdx.x;
  const PairRows pr = load_pair(pairs, p, total_rows, max_frames);
  const int64_t f0 = (int64_t)blockIdx.x * SD_FRAMES;
  if (f0 >= pr.frames) return;  // the whole workgroup: before any barrier
  // this thread's band: its run of bins and where its weights start (the runs lie one after the other)
  int first = 0, count = 0, woff = 0;
  if (tid < n_bands) {
    first = bands[2 * tid];
    count = bands[2 * tid + 1];
    if (first < 0 || count < 0 || first > bins || count > bins - first) count = 0;
  }
  counts[tid] = count;
  for (int e = tid; e < n_weights; e += FD_THREADS) wts[e] = weights[e];
  __syncthreads();
  for (int m = 0; m < tid && m < n_bands; ++m) woff += counts[m];
  if (woff > n_weights - count) count = 0;
  const int64_t f1 = min(f0 + SD_FRAMES, pr.frames);
  for (int64_t f = f0; f < f1; ++f) {
    const float* __restrict__ A = spec + (pr.a + f) * ld;
    const float* __restrict__ B = spec + (pr.b + f) * ld;
    double s[NS] = {0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < bins; k += FD_THREADS) {
      const float xa = amplitude(A[k], A[bins + k]), xb = amplitude(B[k], B[bins + k]);
      amp[0][k] = xa;
      amp[1][k] = xb;
      const double da = (double)xa, db = (double)xb, d = da - db;
      s[1] = fma(d, d, s[1]);
      s[2] = fma(db, db, s[2]);
      s[3] += fabs(log(da) - log(db));
    }
    __syncthreads();
    if (count > 0) {
      float ea = 0.0f, eb = 0.0f;
      for (int i = 0; i < count; ++i) {
        const float w = wts[woff + i];
        ea = __builtin_fmaf(w, amp[0][first + i], ea);
        eb = __builtin_fmaf(w, amp[1][first + i], eb);
      }
      const double ga = (double)ea, gb = (double)eb;
      s[0] = fabs(log10(ga < 1e-10 ? 1e-10 : ga) - log10(gb < 1e-10 ? 1e-10 : gb));
    }
    wave_partials(s, red);
    if (tid == 0) {
      double* out = frame_sums + ((int64_t)p * max_frames + f) * NS;
#pragma unroll
      for (int q = 0; q < NS; ++q) out[q] = fold_sums(red[q]);
    }
    // the next frame's amplitudes are written behind wave_partials' barrier (every band is done with these) and its `red` behind
    // the barrier after them (thread 0 has read these by then)
  }
}

__global__ __launch_bounds__(FD_THREADS) void spectral_reduce_kernel(const double* __restrict__ frame_sums, const int64_t* __restrict__ pairs,
                                                                     int64_t max_frames, double* __restrict__ totals) {
  __shared__ double red[NS][4];
  const int p = blockIdx.x;
  int64_t frames = pairs[3 * p + 2];
  if (frames < 0 || frames > max_frames) frames = 0;
  const double* __restrict__ rows = frame_sums + (int64_t)p * max_frames * NS;
  double s[NS] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t f = threadIdx.x; f < frames; f += FD_THREADS) {
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] += rows[f * NS + q];
  }
  wave_partials(s, red);  // (the only use of red in this kernel)
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NS; ++q) totals[(int64_t)p * NS + q] = fold_sums(red[q]);
  }
}

int frame_reflect(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int64_t max_count, int hop,
                  const int64_t* row_begin, const int64_t* row_begin_host, int64_t total_rows, float* rows, hipStream_t st) {
  TTS_CHECK_ARG(hop >= 4 && hop <= TTS_FIDELITY_MAX_HOP && hop % 4 == 0, "frame_reflect: hop %d is not a multiple of 4 in 4 .. %d", hop,
                TTS_FIDELITY_MAX_HOP);
  int64_t most = 0;
  if (int rc = check_spans("frame_reflect", spans_host, batch, n_samples, [](int64_t c) { return c; }, &most)) return rc;
  TTS_CHECK_ARG(max_count >= most, "frame_reflect: max_count %lld is below the %lld samples of the longest utterance", (long long)max_count,
                (long long)most);
  TTS_CHECK_ARG(total_rows >= 0 && total_rows <= INT64_MAX / TTS_FIDELITY_MAX_HOP, "frame_reflect: total_rows %lld is out of range", (long long)total_rows);
  TTS_CHECK_ARG(batch == 0 || row_begin_host, "frame_reflect: the host copy of row_begin is missing");
  for (int u = 0; u < batch; ++u) {
    const int64_t n = spans_host[2 * u + 1], rb = row_begin_host[u];
    TTS_CHECK_ARG(n > 2 * (int64_t)hop, "frame_reflect: utterance %d has %lld samples, the reflection of %d needs more than that", u, (long long)n,
                  2 * hop);
    const int64_t R = padded_rows(n, hop);
    TTS_CHECK_ARG(rb >= 0 && R <= total_rows && rb <= total_rows - R, "frame_reflect: utterance %d (rows %lld .. %lld) does not lie inside the %lld rows",
                  u, (long long)rb, (long long)(rb + R), (long long)total_rows);
  }
  if (batch == 0) return TTS_OK;
  const int64_t tiles = (padded_rows(most, hop) * hop + FR_TILE - 1) / FR_TILE;
  TTS_CHECK_ARG(tiles <= 0x7fffffff, "frame_reflect: more than 2^31 - 1 workgroups per utterance");
  TTS_CHECK_ARG(x && spans && row_begin && rows, "frame_reflect: null pointer");
  TTS_CHECK_ARG((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "frame_reflect: rows is not 16-byte aligned");
  hipLaunchKernelGGL(frame_reflect_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(FD_THREADS), 0, st, x, n_samples, spans, hop, row_begin,
                     total_rows, rows);
  return launch_status("frame_reflect");
}

static int check_pairs(const char* what, int n_pairs, int64_t max_frames) {
  TTS_CHECK_ARG(n_pairs >= 0 && n_pairs <= 65535, "%s: n_pairs %d is outside 0 .. 65535", what, n_pairs);
  TTS_CHECK_ARG(max_frames >= 1 && max_frames <= INT64_MAX / (65536 * NS * 8), "%s: max_frames %lld is out of range", what, (long long)max_frames);
  return TTS_OK;
}

int spectral_distance(const float* spec, int64_t ld, int bins, int64_t total_rows, const int64_t* pairs, const int64_t* pairs_host, int n_pairs,
                      int64_t max_frames, const int* bands, const int* bands_host, int n_bands, const float* weights, int n_weights,
                      double* frame_sums, hipStream_t st) {
  if (int rc = check_pairs("spectral_distance", n_pairs, max_frames)) return rc;
  TTS_CHECK_ARG(bins >= 1 && bins <= TTS_FIDELITY_MAX_BINS, "spectral_distance: bins %d is outside 1 .. %d", bins, TTS_FIDELITY_MAX_BINS);
  TTS_CHECK_ARG(ld >= 2 * (int64_t)bins, "spectral_distance: ld %lld is below 2 x %d bins", (long long)ld, bins);
  TTS_CHECK_ARG(total_rows >= 0 && total_rows <= INT64_MAX / ld, "spectral_distance: total_rows %lld is out of range", (long long)total_rows);
  TTS_CHECK_ARG(n_bands >= 0 && n_bands <= TTS_FIDELITY_MAX_BANDS, "spectral_distance: n_bands %d is outside 0 .. %d", n_bands, TTS_FIDELITY_MAX_BANDS);
  TTS_CHECK_ARG(n_weights >= 0 && n_weights <= SD_MAX_WEIGHTS, "spectral_distance: n_weights %d is outside 0 .. %d", n_weights, SD_MAX_WEIGHTS);
  TTS_CHECK_ARG(n_bands == 0 || bands_host, "spectral_distance: the host copy of the bands is missing");
  int64_t held = 0;
  for (int m = 0; m < n_bands; ++m) {
    const int first = bands_host[2 * m], count = bands_host[2 * m + 1];
    TTS_CHECK_ARG(first >= 0 && count >= 0 && first <= bins && count <= bins - first, "spectral_distance: band %d (bins %d .. %d) does not lie inside the %d bins",
                  m, first, first + count, bins);
    held += count;
  }
  TTS_CHECK_ARG(held == n_weights, "spectral_distance: the bands hold %lld weights, n_weights is %d", (long long)held, n_weights);
  TTS_CHECK_ARG(n_pairs == 0 || pairs_host, "spectral_distance: the host copy of the pairs is missing");
  int64_t most = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const int64_t a = pairs_host[3 * p], b = pairs_host[3 * p + 1], F = pairs_host[3 * p + 2];
    TTS_CHECK_ARG(F >= 0 && F <= max_frames, "spectral_distance: pair %d has %lld frames, max_frames is %lld", p, (long long)F, (long long)max_frames);
    TTS_CHECK_ARG(a >= 0 && b >= 0 && F <= total_rows && a <= total_rows - F && b <= total_rows - F,
                  "spectral_distance: pair %d (rows %lld and %lld, %lld frames) does not lie inside the spectrum of %lld rows", p, (long long)a, (long long)b,
                  (long long)F, (long long)total_rows);
    if (F > most) most = F;
  }
  const int64_t groups = (most + SD_FRAMES - 1) / SD_FRAMES;
  TTS_CHECK_ARG(groups <= 0x7fffffff, "spectral_distance: more than 2^31 - 1 workgroups per pair");
  if (n_pairs == 0 || groups == 0) return TTS_OK;
  TTS_CHECK_ARG(spec && pairs && frame_sums && (n_bands == 0 || (bands && weights)), "spectral_distance: null pointer");
  hipLaunchKernelGGL(spectral_distance_kernel, dim3((unsigned)groups, (unsigned)n_pairs), dim3(FD_THREADS), 0, st, spec, ld, bins, total_rows, pairs,
                     max_frames, bands, n_bands, weights, n_weights, frame_sums);
  return launch_status("spectral_distance");
}

int spectral_reduce(const double* frame_sums, const int64_t* pairs, int n_pairs, int64_t max_frames, double* totals, hipStream_t st) {
  if (int rc = check_pairs("spectral_reduce", n_pairs, max_frames)) return rc;
  if (n_pairs == 0) return TTS_OK;
  TTS_CHECK_ARG(frame_sums && pairs && totals, "spectral_reduce: null pointer");
  hipLaunchKernelGGL(spectral_reduce_kernel, dim3((unsigned)n_pairs), dim3(FD_THREADS), 0, st, frame_sums, pairs, max_frames, totals);
  return launch_status("spectral_reduce");
}

}  // namespace tts

extern "C" {
int tts_spectral_frames_per_group(void) { return tts::SD_FRAMES; }
int tts_spectral_reduce_sweep(void) { return tts::FD_THREADS; }
int tts_frame_reflect(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, int64_t max_count,
                      int32_t hop, const int64_t* row_begin, const int64_t* row_begin_host, int64_t total_rows, float* rows,
                      tts_stream_t stream) {
  return tts::frame_reflect(x, n_samples, spans, spans_host, batch, max_count, hop, row_begin, row_begin_host, total_rows, rows, (hipStream_t)stream);
}
int tts_spectral_distance(const float* spec, int64_t ld, int32_t bins, int64_t total_rows, const int64_t* pairs, const int64_t* pairs_host,
                          int32_t n_pairs, int64_t max_frames, const int32_t* bands, const int32_t* bands_host, int32_t n_bands,
                          const float* weights, int32_t n_weights, double* frame_sums, tts_stream_t stream) {
  return tts::spectral_distance(spec, ld, bins, total_rows, pairs, pairs_host, n_pairs, max_frames, bands, bands_host, n_bands, weights, n_weights,
                                frame_sums, (hipStream_t)stream);
}
int tts_spectral_reduce(const double* frame_sums, const int64_t* pairs, int32_t n_pairs, int64_t max_frames, double* totals,
                        tts_stream_t stream) {
  return tts::spectral_reduce(frame_sums, pairs, n_pairs, max_frames, totals, (hipStream_t)stream);
}
}
