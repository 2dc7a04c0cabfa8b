// STOI and ESTOI of time-aligned pairs of 10 kHz waveforms (include/toucan_intelligibility.h):
//   tts_stoi_frame_energy  the windowed energy of every frame of the recordings
//   tts_stoi_select        per pair the maximum, the 40 dB mask and its exclusive scan -> the kept frame indices and K
//   tts_stoi_gather        the windowed frames of the compacted signals of both sides, from the wave and the kept list alone
//   tts_stoi_bands         the spectrum of every row -> 15 one-third-octave band values in fp64
//   tts_stoi_segments      the per-segment STOI and ESTOI values; a workgroup stages the frames of its block of segments in LDS
//   tts_stoi_reduce        the per-pair means
// The DFT between gather and bands is tts_conv1d in fp32 (conv1d.hip).  Every sum runs in a fixed order that does not depend on
// the batch; there are no atomics.
#include <math.h>

#include "common.h"
#include "../../include/toucan_intelligibility.h"

namespace tts {

constexpr int ST_THREADS = 256;
constexpr int ST_N = TTS_STOI_FRAME, ST_HOP = TTS_STOI_HOP, ST_BINS = TTS_STOI_BINS, ST_BANDS = TTS_STOI_BANDS, ST_SEG = TTS_STOI_SEGMENT;
constexpr int ST_ENERGY_FRAMES = ST_THREADS / 64;      // frames per workgroup of frame_energy_kernel: one wavefront each
constexpr int ST_PER_THREAD = 4;                       // outputs per thread of gather_kernel: one 16-byte store
constexpr int ST_GATHER_ROWS = ST_THREADS * ST_PER_THREAD / ST_N;
constexpr int ST_BAND_ROWS = ST_THREADS / 16;          // rows per workgroup of bands_kernel: 16 threads a row, 15 of them a band
constexpr int ST_SEG_BLOCK = 32;                       // segments per workgroup of segments_kernel
constexpr int ST_SEG_FRAMES = ST_SEG_BLOCK + ST_SEG - 1;
constexpr double ST_EPS = 2.220446049250313e-16;       // 2^-52
constexpr double ST_CLIP = 6.623413251903491;          // 1 + 10^(15/20)
constexpr double ST_RANGE_DB = 40.0;
__constant__ int st_edges[ST_BANDS + 1] = {TTS_STOI_BAND_EDGES};

__host__ __device__ __forceinline__ int64_t stoi_frames(int64_t n) { return n >= ST_N ? (n - ST_N) / ST_HOP + 1 : 0; }

struct StoiPair {
  int64_t a, b, frames;
};

// a pair that does not lie inside the wave, or has more than max_frames frames, counts as a pair of no frames
__device__ __forceinline__ StoiPair load_stoi_pair(const int64_t* __restrict__ pairs, int p, int64_t n_samples, int64_t max_frames) {
  const int64_t a = pairs[3 * p], b = pairs[3 * p + 1], n = pairs[3 * p + 2];
  StoiPair r = {a, b, 0};
  if (n < 0 || n > n_samples || a < 0 || b < 0 || a > n_samples - n || b > n_samples - n) return r;
  const int64_t F = stoi_frames(n);
  if (F <= max_frames) r.frames = F;
  return r;
}

// the larger of the two; a NaN on either side stays
__device__ __forceinline__ double st_max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double st_level_db(double energy) { return 20.0 * log10(sqrt(energy) + ST_EPS); }

__global__ __launch_bounds__(ST_THREADS) void frame_energy_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ pairs,
                                                                  const float* __restrict__ window, int64_t max_frames,
                                                                  double* __restrict__ energy) {
  const int p = blockIdx.y, lane = threadIdx.x & 63;
  const StoiPair pr = load_stoi_pair(pairs, p, n_samples, max_frames);
  const int64_t f = (int64_t)blockIdx.x * ST_ENERGY_FRAMES + (threadIdx.x >> 6);
  if (f >= pr.frames) return;  // a whole wavefront; there is no barrier
  const float* __restrict__ src = x + pr.a + f * ST_HOP;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < ST_N / 64; ++k) {
    const double v = (double)__fmul_rn(window[lane + 64 * k], src[lane + 64 * k]);
    s = fma(v, v, s);  // (the square of an fp32 value is exact in fp64)
  }
  s = wave_sum(s);
  if (lane == 0) energy[(int64_t)p * max_frames + f] = s;
}

__global__ __launch_bounds__(ST_THREADS) void select_kernel(const double* __restrict__ energy, const int64_t* __restrict__ pairs, int64_t n_samples,
                                                            int64_t max_frames, int* __restrict__ kept, int* __restrict__ counts) {
  __shared__ double top[ST_THREADS / 64];
  __shared__ int wave_count[ST_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t F = load_stoi_pair(pairs, p, n_samples, max_frames).frames;  // uniform
  const double* __restrict__ e = energy + (int64_t)p * max_frames;
  int* __restrict__ out = kept + (int64_t)p * max_frames;
  double mx = -INFINITY;
  for (int64_t f = tid; f < F; f += ST_THREADS) mx = st_max_nan(mx, st_level_db(e[f]));
  // the butterfly and the left fold of wave_ops.h with one barrier: top is written once, before any other barrier of the kernel
  mx = wave_fold(mx, st_max_nan);
  if (lane == 0) top[wv] = mx;
  __syncthreads();
  mx = fold_left(top, st_max_nan);
  const double threshold = mx - ST_RANGE_DB;
  int64_t run = 0;  // frames kept in the sweeps before this one (uniform)
  for (int64_t f0 = 0; f0 < F; f0 += ST_THREADS) {
    const int64_t f = f0 + tid;
    const bool keep = f < F && st_level_db(e[f]) > threshold;
    const unsigned long long ballot = __ballot(keep);
    if (lane == 0) wave_count[wv] = __popcll(ballot);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < ST_THREADS / 64; ++k) {
      const int c = wave_count[k];
      before += k < wv ? c : 0;
      all += c;
    }
    if (keep) out[run + before + __popcll(ballot & ((1ull << lane) - 1ull))] = (int)f;
    run += all;
    __syncthreads();  // wave_count is rewritten by the next sweep
  }
  if (tid == 0) counts[p] = (int)run;
}

__global__ __launch_bounds__(ST_THREADS) void gather_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ pairs,
                                                            const float* __restrict__ window, int64_t max_frames, const int* __restrict__ kept,
                                                            const int* __restrict__ counts, const int64_t* __restrict__ row_begin,
                                                            int64_t total_rows, float* __restrict__ rows) {
  const int p = blockIdx.y, side = blockIdx.z;
  const StoiPair pr = load_stoi_pair(pairs, p, n_samples, max_frames);
  const int64_t F = pr.frames, rb = row_begin[2 * p + side];
  if (F == 0 || rb < 0 || F > total_rows || rb > total_rows - F) return;
  const int64_t j0 = ((int64_t)blockIdx.x * ST_THREADS + threadIdx.x) * ST_PER_THREAD;
  const int64_t m = j0 / ST_N;
  if (m >= F) return;
  int64_t K = counts[p];
  if (K < 0 || K > F) K = 0;
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (m < K) {
    const int i0 = (int)(j0 % ST_N);            // a multiple of 4: the four outputs lie in one half of the row
    const int64_t q = m + (i0 >= ST_HOP), r0 = i0 & (ST_HOP - 1);
    const float* __restrict__ src = x + (side ? pr.b : pr.a);
    const int* __restrict__ idx = kept + (int64_t)p * max_frames;
    // frame q - 1 gives its second half, frame q its first: both reads stay inside [0, 128 (F - 1) + 256) <= n
    const bool has_prev = q >= 1, has_cur = q < K;
    const int64_t fp = has_prev ? min(max((int64_t)idx[q - 1], (int64_t)0), F - 1) : 0, fc = has_cur ? min(max((int64_t)idx[q], (int64_t)0), F - 1) : 0;
#pragma unroll
    for (int e = 0; e < ST_PER_THREAD; ++e) {
      const int r = (int)r0 + e;
      const float prev = has_prev ? __fmul_rn(window[r + ST_HOP], src[fp * ST_HOP + ST_HOP + r]) : 0.0f;
      const float cur = has_cur ? __fmul_rn(window[r], src[fc * ST_HOP + r]) : 0.0f;
      v[e] = __fmul_rn(window[i0 + e], __fadd_rn(__fadd_rn(0.0f, prev), cur));
    }
  }
  *reinterpret_cast<f32x4*>(rows + rb * ST_N + j0) = v;  // (rb 256 + j0) is a multiple of 4 and `rows` 16-byte aligned
}

__global__ __launch_bounds__(ST_THREADS) void bands_kernel(const float* __restrict__ spec, int64_t ld, int64_t total_rows, double* __restrict__ bands) {
  const int j = threadIdx.x & 15;
  const int64_t r = (int64_t)blockIdx.x * ST_BAND_ROWS + (threadIdx.x >> 4);
  if (r >= total_rows || j >= ST_BANDS) return;
  const float* __restrict__ re = spec + r * ld;
  const float* __restrict__ im = re + ST_BINS;
  double s = 0.0;
  for (int k = st_edges[j]; k < st_edges[j + 1]; ++k) {
    const double a = (double)re[k], b = (double)im[k];
    s = fma(a, a, s);
    s = fma(b, b, s);
  }
  bands[r * ST_BANDS + j] = sqrt(s);
}

// min(a, b) that keeps a NaN of either side
__device__ __forceinline__ double st_min_nan(double a, double b) { return (a < b || a != a) ? a : b; }

__global__ __launch_bounds__(ST_THREADS) void segments_kernel(const double* __restrict__ bands, int64_t total_rows, const int64_t* __restrict__ row_begin,
                                                              const int* __restrict__ counts, int64_t max_frames, int64_t max_segments,
                                                              double* __restrict__ segments) {
  // frames [f][j]: thread (j, s) of the first phase reads element 15 (s + n) + j = its own index + 15 n, consecutive 8-byte words
  // over the lanes, and the statistics [j][s] are read along s by the second phase: neither is a bank conflict.  The second
  // phase's reads of the frames are 15 doubles apart over the lanes (s fastest), a 2-way conflict on 64 banks of 4 bytes.
  __shared__ double xs[ST_SEG_FRAMES * ST_BANDS], ys[ST_SEG_FRAMES * ST_BANDS];
  __shared__ double mean_x[ST_BANDS * ST_SEG_BLOCK], div_x[ST_BANDS * ST_SEG_BLOCK], mean_y[ST_BANDS * ST_SEG_BLOCK], div_y[ST_BANDS * ST_SEG_BLOCK];
  __shared__ double d_band[ST_BANDS * ST_SEG_BLOCK];
  __shared__ double d_col[ST_SEG * ST_SEG_BLOCK];
  const int p = blockIdx.y, tid = threadIdx.x;
  int64_t M = counts[p];
  const int64_t ra = row_begin[2 * p], rb = row_begin[2 * p + 1];
  if (M < 0 || M > max_frames || M > total_rows || ra < 0 || rb < 0 || ra > total_rows - M || rb > total_rows - M) M = 0;
  const int64_t S = M - (ST_SEG - 1), s0 = (int64_t)blockIdx.x * ST_SEG_BLOCK;
  if (s0 >= S) return;  // the whole workgroup: before any barrier
  const int n_seg = (int)min((int64_t)ST_SEG_BLOCK, S - s0), n_fr = n_seg + ST_SEG - 1;
  const double* __restrict__ A = bands + (ra + s0) * ST_BANDS;
  const double* __restrict__ B = bands + (rb + s0) * ST_BANDS;
  for (int e = tid; e < ST_SEG_FRAMES * ST_BANDS; e += ST_THREADS) {
    const bool in = e < n_fr * ST_BANDS;
    xs[e] = in ? A[e] : 0.0;
    ys[e] = in ? B[e] : 0.0;
  }
  __syncthreads();
  // phase 1, one (band, segment) per thread: STOI's d, and mean and divisor of the band's row of the ESTOI matrices
  for (int item = tid; item < ST_BANDS * n_seg; item += ST_THREADS) {
    const int j = item % ST_BANDS, s = item / ST_BANDS;
    const double* __restrict__ px = xs + s * ST_BANDS + j;
    const double* __restrict__ py = ys + s * ST_BANDS + j;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0;
    for (int n = 0; n < ST_SEG; ++n) {
      const double a = px[n * ST_BANDS], b = py[n * ST_BANDS];
      sx += a;
      sy += b;
      sxx += a * a;
      syy += b * b;
    }
    const double alpha = sqrt(sxx) / (sqrt(syy) + ST_EPS);
    double sc = 0.0;
    for (int n = 0; n < ST_SEG; ++n) sc += st_min_nan(alpha * py[n * ST_BANDS], ST_CLIP * px[n * ST_BANDS]);
    const double mx = sx / ST_SEG, my = sy / ST_SEG, mc = sc / ST_SEG;
    double vxx = 0.0, vyy = 0.0, vcc = 0.0, vxc = 0.0;
    for (int n = 0; n < ST_SEG; ++n) {
      const double a = px[n * ST_BANDS], b = py[n * ST_BANDS];
      const double da = a - mx, db = b - my, dc = st_min_nan(alpha * b, ST_CLIP * a) - mc;
      vxx += da * da;
      vyy += db * db;
      vcc += dc * dc;
      vxc += da * dc;
    }
    d_band[j * ST_SEG_BLOCK + s] = vxc / (sqrt(vxx) * sqrt(vcc) + ST_EPS);
    mean_x[j * ST_SEG_BLOCK + s] = mx;
    div_x[j * ST_SEG_BLOCK + s] = sqrt(vxx) + ST_EPS;
    mean_y[j * ST_SEG_BLOCK + s] = my;
    div_y[j * ST_SEG_BLOCK + s] = sqrt(vyy) + ST_EPS;
  }
  __syncthreads();
  // phase 2, one (segment, column) per thread: the column of both row-normalised matrices in registers, normalised, multiplied
  for (int item = tid; item < ST_SEG * ST_SEG_BLOCK; item += ST_THREADS) {
    const int s = item % ST_SEG_BLOCK, n = item / ST_SEG_BLOCK;
    if (s >= n_seg) continue;
    double a[ST_BANDS], b[ST_BANDS];
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) {
      a[j] = (xs[(s + n) * ST_BANDS + j] - mean_x[j * ST_SEG_BLOCK + s]) / div_x[j * ST_SEG_BLOCK + s];
      b[j] = (ys[(s + n) * ST_BANDS + j] - mean_y[j * ST_SEG_BLOCK + s]) / div_y[j * ST_SEG_BLOCK + s];
      sa += a[j];
      sb += b[j];
    }
    const double ma = sa / ST_BANDS, mb = sb / ST_BANDS;
    double vaa = 0.0, vbb = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) {
      a[j] -= ma;
      b[j] -= mb;
      vaa += a[j] * a[j];
      vbb += b[j] * b[j];
    }
    const double da = sqrt(vaa) + ST_EPS, db = sqrt(vbb) + ST_EPS;
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) dot += (a[j] / da) * (b[j] / db);
    d_col[n * ST_SEG_BLOCK + s] = dot;
  }
  __syncthreads();
  if (tid < n_seg) {
    double st = 0.0, es = 0.0;
    for (int j = 0; j < ST_BANDS; ++j) st += d_band[j * ST_SEG_BLOCK + tid];
    for (int n = 0; n < ST_SEG; ++n) es += d_col[n * ST_SEG_BLOCK + tid];
    double* out = segments + ((int64_t)p * max_segments + s0 + tid) * 2;
    out[0] = st / ST_BANDS;
    out[1] = es / ST_SEG;
  }
}

__global__ __launch_bounds__(ST_THREADS) void stoi_reduce_kernel(const double* __restrict__ segments, const int* __restrict__ counts, int64_t max_frames,
                                                                 int64_t max_segments, double* __restrict__ totals) {
  __shared__ double red[2][ST_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  int64_t M = counts[p];
  if (M < 0 || M > max_frames) M = 0;
  const int64_t S = M - (ST_SEG - 1);  // (<= max_segments)
  const double* __restrict__ rows = segments + (int64_t)p * max_segments * 2;
  double s[2] = {0.0, 0.0};
  for (int64_t k = tid; k < S; k += ST_THREADS) {
    s[0] += rows[2 * k];
    s[1] += rows[2 * k + 1];
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    s[q] = wave_sum(s[q]);
    if ((tid & 63) == 0) red[q][tid >> 6] = s[q];
  }
  __syncthreads();  // one barrier: the only use of red in this kernel
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      totals[2 * (int64_t)p + q] = S > 0 ? fold_left(red[q], [](double a, double b) { return a + b; }) / (double)S : (double)NAN;
  }
}

// the checks of every entry that reads the pairs -> *most = the frames of the longest pair
static int check_stoi_pairs(const char* what, const int64_t* pairs_host, int n_pairs, int64_t n_samples, int64_t max_frames, int64_t* most) {
  TTS_CHECK_ARG(n_pairs >= 0 && n_pairs <= 65535, "%s: n_pairs %d is outside 0 .. 65535", what, n_pairs);
  TTS_CHECK_ARG(n_samples >= 0, "%s: n_samples is negative", what);
  TTS_CHECK_ARG(max_frames >= 1 && max_frames <= TTS_STOI_MAX_FRAMES, "%s: max_frames %lld is outside 1 .. %d", what, (long long)max_frames,
                TTS_STOI_MAX_FRAMES);
  TTS_CHECK_ARG(n_pairs == 0 || pairs_host, "%s: the host copy of the pairs is missing", what);
  *most = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const int64_t a = pairs_host[3 * p], b = pairs_host[3 * p + 1], n = pairs_host[3 * p + 2];
    TTS_CHECK_ARG(n >= 0 && n <= n_samples && a >= 0 && b >= 0 && a <= n_samples - n && b <= n_samples - n,
                  "%s: pair %d (samples %lld .. and %lld .., %lld each) does not lie inside the wave of %lld samples", what, p, (long long)a, (long long)b,
                  (long long)n, (long long)n_samples);
    const int64_t F = stoi_frames(n);
    TTS_CHECK_ARG(F <= max_frames, "%s: pair %d has %lld frames, max_frames is %lld", what, p, (long long)F, (long long)max_frames);
    if (F > *most) *most = F;
  }
  return TTS_OK;
}

static int check_stoi_rows(const char* what, const int64_t* row_begin_host, const int64_t* frames_host, const int64_t* pairs_host, int n_pairs,
                           int64_t max_frames, int64_t total_rows) {
  TTS_CHECK_ARG(total_rows >= 0 && total_rows <= INT64_MAX / 4096, "%s: total_rows %lld is out of range", what, (long long)total_rows);
  TTS_CHECK_ARG(n_pairs == 0 || row_begin_host, "%s: the host copy of row_begin is missing", what);
  for (int p = 0; p < n_pairs; ++p) {
    const int64_t F = frames_host ? frames_host[p] : stoi_frames(pairs_host[3 * p + 2]);
    TTS_CHECK_ARG(F >= 0 && F <= max_frames, "%s: pair %d has %lld frames, max_frames is %lld", what, p, (long long)F, (long long)max_frames);
    for (int side = 0; side < 2; ++side) {
      const int64_t rb = row_begin_host[2 * p + side];
      TTS_CHECK_ARG(rb >= 0 && F <= total_rows && rb <= total_rows - F, "%s: pair %d (rows %lld .. %lld) does not lie inside the %lld rows", what, p,
                    (long long)rb, (long long)(rb + F), (long long)total_rows);
    }
  }
  return TTS_OK;
}

int stoi_frame_energy(const float* x, int64_t n_samples, const int64_t* pairs, const int64_t* pairs_host, int n_pairs, const float* window,
                      int64_t max_frames, double* energy, hipStream_t st) {
  int64_t most = 0;
  if (int rc = check_stoi_pairs("stoi_frame_energy", pairs_host, n_pairs, n_samples, max_frames, &most)) return rc;
  if (n_pairs == 0 || most == 0) return TTS_OK;
  TTS_CHECK_ARG(x && pairs && window && energy, "stoi_frame_energy: null pointer");
  const int64_t groups = (most + ST_ENERGY_FRAMES - 1) / ST_ENERGY_FRAMES;
  hipLaunchKernelGGL(frame_energy_kernel, dim3((unsigned)groups, (unsigned)n_pairs), dim3(ST_THREADS), 0, st, x, n_samples, pairs, window, max_frames,
                     energy);
  return launch_status("stoi_frame_energy");
}

int stoi_select(const double* energy, const int64_t* pairs, const int64_t* pairs_host, int n_pairs, int64_t n_samples, int64_t max_frames, int* kept,
                int* counts, hipStream_t st) {
  int64_t most = 0;
  if (int rc = check_stoi_pairs("stoi_select", pairs_host, n_pairs, n_samples, max_frames, &most)) return rc;
  if (n_pairs == 0) return TTS_OK;
  TTS_CHECK_ARG(energy && pairs && kept && counts, "stoi_select: null pointer");
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)n_pairs), dim3(ST_THREADS), 0, st, energy, pairs, n_samples, max_frames, kept, counts);
  return launch_status("stoi_select");
}

int stoi_gather(const float* x, int64_t n_samples, const int64_t* pairs, const int64_t* pairs_host, int n_pairs, const float* window,
                int64_t max_frames, const int* kept, const int* counts, const int64_t* row_begin, const int64_t* row_begin_host, int64_t total_rows,
                float* rows, hipStream_t st) {
  int64_t most = 0;
  if (int rc = check_stoi_pairs("stoi_gather", pairs_host, n_pairs, n_samples, max_frames, &most)) return rc;
  if (int rc = check_stoi_rows("stoi_gather", row_begin_host, nullptr, pairs_host, n_pairs, max_frames, total_rows)) return rc;
  if (n_pairs == 0 || most == 0) return TTS_OK;
  TTS_CHECK_ARG(x && pairs && window && kept && counts && row_begin && rows, "stoi_gather: null pointer");
  TTS_CHECK_ARG((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "stoi_gather: rows is not 16-byte aligned");
  const int64_t groups = (most + ST_GATHER_ROWS - 1) / ST_GATHER_ROWS;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)groups, (unsigned)n_pairs, 2), dim3(ST_THREADS), 0, st, x, n_samples, pairs, window, max_frames, kept,
                     counts, row_begin, total_rows, rows);
  return launch_status("stoi_gather");
}

int stoi_bands(const float* spec, int64_t ld, int64_t total_rows, double* bands, hipStream_t st) {
  TTS_CHECK_ARG(ld >= 2 * ST_BINS && ld <= 65536, "stoi_bands: ld %lld is outside %d .. 65536", (long long)ld, 2 * ST_BINS);
  TTS_CHECK_ARG(total_rows >= 0 && total_rows <= 0x7fffffffll * ST_BAND_ROWS, "stoi_bands: total_rows %lld is out of range", (long long)total_rows);
  if (total_rows == 0) return TTS_OK;
  TTS_CHECK_ARG(spec && bands, "stoi_bands: null pointer");
  const int64_t groups = (total_rows + ST_BAND_ROWS - 1) / ST_BAND_ROWS;
  hipLaunchKernelGGL(bands_kernel, dim3((unsigned)groups), dim3(ST_THREADS), 0, st, spec, ld, total_rows, bands);
  return launch_status("stoi_bands");
}

static int check_stoi_counts(const char* what, int n_pairs, int64_t max_frames) {
  TTS_CHECK_ARG(n_pairs >= 0 && n_pairs <= 65535, "%s: n_pairs %d is outside 0 .. 65535", what, n_pairs);
  TTS_CHECK_ARG(max_frames >= 1 && max_frames <= TTS_STOI_MAX_FRAMES, "%s: max_frames %lld is outside 1 .. %d", what, (long long)max_frames,
                TTS_STOI_MAX_FRAMES);
  return TTS_OK;
}

static int64_t stoi_max_segments(int64_t max_frames) { return max_frames >= ST_SEG ? max_frames - (ST_SEG - 1) : 1; }

int stoi_segments(const double* bands, int64_t total_rows, const int64_t* row_begin, const int64_t* row_begin_host, const int64_t* frames_host,
                  const int* counts, int n_pairs, int64_t max_frames, double* segments, hipStream_t st) {
  if (int rc = check_stoi_counts("stoi_segments", n_pairs, max_frames)) return rc;
  TTS_CHECK_ARG(n_pairs == 0 || frames_host, "stoi_segments: the host copy of the frame counts is missing");
  if (int rc = check_stoi_rows("stoi_segments", row_begin_host, frames_host, nullptr, n_pairs, max_frames, total_rows)) return rc;
  int64_t most = 0;
  for (int p = 0; p < n_pairs; ++p) most = frames_host[p] > most ? frames_host[p] : most;
  if (n_pairs == 0 || most < ST_SEG) return TTS_OK;
  TTS_CHECK_ARG(bands && row_begin && counts && segments, "stoi_segments: null pointer");
  const int64_t groups = (most - (ST_SEG - 1) + ST_SEG_BLOCK - 1) / ST_SEG_BLOCK;
  hipLaunchKernelGGL(segments_kernel, dim3((unsigned)groups, (unsigned)n_pairs), dim3(ST_THREADS), 0, st, bands, total_rows, row_begin, counts, max_frames,
                     stoi_max_segments(max_frames), segments);
  return launch_status("stoi_segments");
}

int stoi_reduce(const double* segments, const int* counts, int n_pairs, int64_t max_frames, double* totals, hipStream_t st) {
  if (int rc = check_stoi_counts("stoi_reduce", n_pairs, max_frames)) return rc;
  if (n_pairs == 0) return TTS_OK;
  TTS_CHECK_ARG(segments && counts && totals, "stoi_reduce: null pointer");
  hipLaunchKernelGGL(stoi_reduce_kernel, dim3((unsigned)n_pairs), dim3(ST_THREADS), 0, st, segments, counts, max_frames, stoi_max_segments(max_frames),
                     totals);
  return launch_status("stoi_reduce");
}

}  // namespace tts

extern "C" {
int tts_stoi_select_sweep(void) { return tts::ST_THREADS; }
int tts_stoi_segments_per_group(void) { return tts::ST_SEG_BLOCK; }
int tts_stoi_frame_energy(const float* x, int64_t n_samples, const int64_t* pairs, const int64_t* pairs_host, int32_t n_pairs,
                          const float* window, int64_t max_frames, double* energy, tts_stream_t stream) {
  return tts::stoi_frame_energy(x, n_samples, pairs, pairs_host, n_pairs, window, max_frames, energy, (hipStream_t)stream);
}
int tts_stoi_select(const double* energy, const int64_t* pairs, const int64_t* pairs_host, int32_t n_pairs, int64_t n_samples,
                    int64_t max_frames, int32_t* kept, int32_t* counts, tts_stream_t stream) {
  return tts::stoi_select(energy, pairs, pairs_host, n_pairs, n_samples, max_frames, kept, counts, (hipStream_t)stream);
}
int tts_stoi_gather(const float* x, int64_t n_samples, const int64_t* pairs, const int64_t* pairs_host, int32_t n_pairs,
                    const float* window, int64_t max_frames, const int32_t* kept, const int32_t* counts, const int64_t* row_begin,
                    const int64_t* row_begin_host, int64_t total_rows, float* rows, tts_stream_t stream) {
  return tts::stoi_gather(x, n_samples, pairs, pairs_host, n_pairs, window, max_frames, kept, counts, row_begin, row_begin_host, total_rows, rows,
                          (hipStream_t)stream);
}
int tts_stoi_bands(const float* spec, int64_t ld, int64_t total_rows, double* bands, tts_stream_t stream) {
  return tts::stoi_bands(spec, ld, total_rows, bands, (hipStream_t)stream);
}
int tts_stoi_segments(const double* bands, int64_t total_rows, const int64_t* row_begin, const int64_t* row_begin_host,
                      const int64_t* frames_host, const int32_t* counts, int32_t n_pairs, int64_t max_frames, double* segments,
                      tts_stream_t stream) {
  return tts::stoi_segments(bands, total_rows, row_begin, row_begin_host, frames_host, counts, n_pairs, max_frames, segments, (hipStream_t)stream);
}
int tts_stoi_reduce(const double* segments, const int32_t* counts, int32_t n_pairs, int64_t max_frames, double* totals,
                    tts_stream_t stream) {
  return tts::stoi_reduce(segments, counts, n_pairs, max_frames, totals, (hipStream_t)stream);
}
}
