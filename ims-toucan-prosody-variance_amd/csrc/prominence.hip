// Word prominence and boundary strength from the wavelet transform of three prosodic tracks (include/toucan_prominence.h, DESIGN.md
// section 24):
//   tts_prominence_channels  per utterance ln f0, ln energy and ln phoneme duration per frame, gaps filled, z-normalised, in fp64
//   tts_prominence_cwt       the Mexican-hat transform of the three channels at six dyadic scales, a tile and its halo in LDS
//   tts_prominence_units     the band sums, the composite, per unit its maximum and mean, between consecutive peaks the valley
// Every sum runs in a fixed order that depends on its utterance alone; there are no atomics, and nothing is contracted that the
// header does not write as a fused multiply-add.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/toucan_prominence.h"

#pragma clang fp contract(off)

namespace tts {

constexpr int PM_THREADS = TTS_PROMINENCE_TILE;
constexpr int PM_WAVES = PM_THREADS / 64;
constexpr int PM_CH = TTS_PROMINENCE_CHANNELS, PM_SCALES = TTS_PROMINENCE_SCALES, PM_COLS = TTS_PROMINENCE_COLUMNS;
constexpr int PM_MAX_TAPS = TTS_PROMINENCE_MAX_TAPS, PM_TABLE_LD = TTS_PROMINENCE_TABLE_LD;
constexpr int PM_MAX_HALO = (PM_MAX_TAPS - 1) / 2;          // 8 s_5 = 512 frames on either side
constexpr int PM_WINDOW = PM_THREADS + 2 * PM_MAX_HALO;     // 1280 frames of a channel in LDS at the widest scale
constexpr int PM_NONE = INT_MAX;                            // "no valid frame to the right" (exact as a double)
static_assert(PM_THREADS == 256 && PM_WAVES == 4, "the reductions (wave_ops.h) fold four wavefronts");

struct PmUtt {
  int64_t first, T, ph0, nph, un0, nun;
};

// an utterance that does not lie inside the arrays counts as one of no frames, phonemes and units; a table the kernel does not
// read is given as -1 rows and not looked at
__device__ __forceinline__ PmUtt load_pm_utt(const int64_t* __restrict__ utts, int u, int64_t total_frames, int64_t n_phones, int64_t n_units) {
  const int64_t* r = utts + (int64_t)u * TTS_PROMINENCE_UTT_COLUMNS;
  PmUtt v = {r[0], r[1], r[2], r[3], r[4], r[5]};
  const bool ok = v.T >= 1 && v.T <= TTS_PROMINENCE_MAX_FRAMES && v.first >= 0 && v.T <= total_frames && v.first <= total_frames - v.T &&
                  (n_phones < 0 || (v.ph0 >= 0 && v.nph >= 0 && v.nph <= n_phones && v.ph0 <= n_phones - v.nph)) &&
                  (n_units < 0 || (v.un0 >= 0 && v.nun >= 0 && v.nun <= n_units && v.un0 <= n_units - v.nun));
  if (!ok) v.T = v.nph = v.nun = 0;
  return v;
}

// The value of channel c at frame t of the utterance and whether the frame is valid (f0, en: the utterance's own frames; ph: its
// own phoneme rows).  c is uniform over the workgroup.
__device__ __forceinline__ bool pm_value(int c, int t, const float* __restrict__ f0, const float* __restrict__ en, const int32_t* __restrict__ ph,
                                         int64_t nph, double floor_e, double* v) {
  *v = 0.0;
  if (c == 0) {
    const float f = f0[t];
    if (!(f > 0.0f && f < INFINITY)) return false;
    *v = log((double)f);
    return true;
  }
  if (c == 1) {
    const double e = (double)en[t];
    *v = log(e > floor_e ? e : floor_e);
    return true;
  }
  int64_t lo = 0, hi = nph;  // -> the number of phonemes that begin at or before t
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ph[3 * mid] <= t) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return false;
  const int b = ph[3 * (lo - 1)], e = ph[3 * (lo - 1) + 1];
  if (t >= e || ph[3 * (lo - 1) + 2] == 0) return false;  // (b <= t < e: e - b >= 1)
  *v = log((double)(e - b));
  return true;
}

__global__ __launch_bounds__(PM_THREADS) void prominence_channels_kernel(const float* __restrict__ f0, const float* __restrict__ energy, int64_t total_frames,
                                                                         const int64_t* __restrict__ utts, const int32_t* __restrict__ phones,
                                                                         int64_t n_phones, double* x) {
  __shared__ double red_d[PM_WAVES];
  __shared__ float red_f[PM_WAVES];
  __shared__ int red_i[PM_WAVES];
  const int tid = threadIdx.x;
  const PmUtt utt = load_pm_utt(utts, blockIdx.x, total_frames, n_phones, -1);  // uniform
  const int T = (int)utt.T;
  if (T == 0) return;  // the whole workgroup, before any barrier
  const float* __restrict__ f0u = f0 + utt.first;
  const float* __restrict__ enu = energy + utt.first;
  const int32_t* __restrict__ ph = phones + 3 * utt.ph0;
  const int chunks = (T + PM_THREADS - 1) / PM_THREADS;
  // the energy floor: the maximum does not depend on an order
  float top = 0.0f;
  for (int t = tid; t < T; t += PM_THREADS) top = fmaxf(top, enu[t]);
  // one barrier (red_f is written once in this kernel); the left fold equals the (0,1),(2,3) one: top >= 0 and never a NaN
  top = wave_max(top);
  if ((tid & 63) == 0) red_f[tid >> 6] = top;
  __syncthreads();
  top = fold_left(red_f, [](float a, float b) { return fmaxf(a, b); });
  const double lowest = (double)FLT_MIN, scaled = 1e-3 * (double)top;
  const double floor_e = scaled > lowest ? scaled : lowest;
  for (int c = 0; c < PM_CH; ++c) {
    double* xc = x + (int64_t)c * total_frames + utt.first;  // (read back below: not __restrict__)
    // backward: a valid frame gets its value, an invalid one the index of the nearest valid frame to its right
    int carry = PM_NONE;
    for (int q = chunks - 1; q >= 0; --q) {
      const int t = q * PM_THREADS + tid;
      double v;
      const bool in = t < T, valid = in && pm_value(c, t, f0u, enu, ph, utt.nph, floor_e, &v);
      int all;
      const int r = min(block_scan_backward(valid ? t : PM_NONE, red_i, &all, [](int a, int b) { return min(a, b); }), carry);
      if (in) xc[t] = valid ? v : (double)r;
      carry = min(carry, all);
    }
    __syncthreads();  // the values of the valid frames are read by other threads below
    // forward: the nearest valid frame to the left, and the fill
    carry = -1;
    for (int q = 0; q < chunks; ++q) {
      const int t = q * PM_THREADS + tid;
      double v;
      const bool in = t < T, valid = in && pm_value(c, t, f0u, enu, ph, utt.nph, floor_e, &v);
      int all;
      const int l = max(block_scan_forward(valid ? t : -1, red_i, &all, [](int a, int b) { return max(a, b); }), carry);
      if (in && !valid) {
        const int r = (int)xc[t];
        double y = 0.0;
        if (l >= 0 && r != PM_NONE) {
          const double a = xc[l], b = xc[r];
          y = a + (b - a) * ((double)(t - l) / (double)(r - l));
        } else if (l >= 0) {
          y = xc[l];
        } else if (r != PM_NONE) {
          y = xc[r];
        }
        xc[t] = y;  // (no thread reads an invalid frame of another)
      }
      carry = max(carry, all);
    }
    __syncthreads();
    double s = 0.0;
    for (int t = tid; t < T; t += PM_THREADS) s += xc[t];
    const double mean = block_sum(s, red_d) / (double)T;
    s = 0.0;
    for (int t = tid; t < T; t += PM_THREADS) {
      const double d = xc[t] - mean;
      s += d * d;
    }
    const double sd = sqrt(block_sum(s, red_d) / (double)T);
    const double am = fabs(mean);
    const bool flat = !(sd > 1e-12 * (am > 1.0 ? am : 1.0));
    for (int t = tid; t < T; t += PM_THREADS) xc[t] = flat ? 0.0 : (xc[t] - mean) / sd;  // (its own frames only)
  }
}

__global__ __launch_bounds__(PM_THREADS) void prominence_cwt_kernel(const double* __restrict__ x, int64_t total_frames, const int64_t* __restrict__ utts,
                                                                    const double* __restrict__ table, double* __restrict__ w) {
  __shared__ double win[PM_CH][PM_WINDOW];
  __shared__ double taps[PM_MAX_TAPS];
  const int tid = threadIdx.x, j = blockIdx.y;
  const PmUtt utt = load_pm_utt(utts, blockIdx.z, total_frames, -1, -1);
  const int T = (int)utt.T, tile0 = blockIdx.x * PM_THREADS;
  if (tile0 >= T) return;  // the whole workgroup, before the barrier
  const int halo = 8 << (j + 1), n_taps = 2 * halo + 1;
  for (int i = tid; i < PM_THREADS + 2 * halo; i += PM_THREADS) {
    const int t = tile0 - halo + i;
    const bool in = t >= 0 && t < T;
#pragma unroll
    for (int c = 0; c < PM_CH; ++c) win[c][i] = in ? x[(int64_t)c * total_frames + utt.first + t] : 0.0;
  }
  for (int i = tid; i < n_taps; i += PM_THREADS) taps[i] = table[j * PM_TABLE_LD + i];
  const double norm = table[j * PM_TABLE_LD + PM_MAX_TAPS];
  __syncthreads();
  const int t = tile0 + tid;
  if (t >= T) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i = 0; i < n_taps; ++i) {  // lane l reads word l + i of each channel: consecutive 8-byte words; the tap is a broadcast
    const double p = taps[i];
    a0 = fma(win[0][tid + i], p, a0);
    a1 = fma(win[1][tid + i], p, a1);
    a2 = fma(win[2][tid + i], p, a2);
  }
  double* __restrict__ out = w + (int64_t)j * total_frames + utt.first + t;
  out[0] = norm * a0;
  out[(int64_t)PM_SCALES * total_frames] = norm * a1;
  out[2 * (int64_t)PM_SCALES * total_frames] = norm * a2;
}

struct PmMix {
  double weight[PM_CH];
  int j_lo, j_hi;
};

// P[t] and its three parts at frame g of the packed arrays
__device__ __forceinline__ double pm_composite(const double* __restrict__ w, int64_t total_frames, int64_t g, const PmMix& m, double* parts) {
#pragma unroll
  for (int c = 0; c < PM_CH; ++c) {
    double s = 0.0;
    for (int j = m.j_lo; j <= m.j_hi; ++j) s += w[((int64_t)c * PM_SCALES + j) * total_frames + g];
    parts[c] = m.weight[c] * s;
  }
  return (parts[0] + parts[1]) + parts[2];
}

__global__ __launch_bounds__(PM_THREADS) void prominence_units_kernel(const double* __restrict__ w, int64_t total_frames, const int64_t* __restrict__ utts,
                                                                      const int32_t* __restrict__ units, int64_t n_units, PmMix mix, double* rows,
                                                                      double* __restrict__ p) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const PmUtt utt = load_pm_utt(utts, blockIdx.x, total_frames, -1, n_units);
  const int T = (int)utt.T;
  if (T == 0) return;  // the whole workgroup, before the barrier
  double parts[PM_CH];
  if (p)
    for (int t = tid; t < T; t += PM_THREADS) p[utt.first + t] = pm_composite(w, total_frames, utt.first + t, mix, parts);
  const int32_t* __restrict__ un = units + 2 * utt.un0;
  double* out = rows + utt.un0 * PM_COLS;  // (the peaks are read back below: not __restrict__)
  // one wavefront per unit: the maximum with the first frame that attains it, and the mean
  for (int64_t k = wv; k < utt.nun; k += PM_WAVES) {
    const int b = min(max(un[2 * k], 0), T), e = min(max(un[2 * k + 1], b), T);
    double best = -INFINITY, sum = 0.0;
    int at = PM_NONE;
    for (int t = b + lane; t < e; t += 64) {
      const double v = pm_composite(w, total_frames, utt.first + t, mix, parts);
      sum += v;
      if (v > best) {  // (ascending t: the first of equal values stays)
        best = v;
        at = t;
      }
    }
    sum = wave_sum(sum);
    wave_arg_max(best, at);
    if (lane == 0) {
      double* row = out + k * PM_COLS;
      const bool found = at != PM_NONE;
      if (found) pm_composite(w, total_frames, utt.first + at, mix, parts);
      row[0] = found ? best : (double)NAN;
      row[1] = found ? (double)at : -1.0;
      row[2] = found ? sum / (double)(e - b) : (double)NAN;
#pragma unroll
      for (int c = 0; c < PM_CH; ++c) row[3 + c] = found ? parts[c] : (double)NAN;
      row[6] = (double)NAN;
      row[7] = -1.0;
    }
  }
  __syncthreads();  // every peak is written (outside any divergent branch: the loops above end for all)
  // one wavefront per unit: the valley between its peak and the peak of the next unit that has one
  for (int64_t k = wv; k < utt.nun; k += PM_WAVES) {
    const int from = (int)out[k * PM_COLS + 1];
    if (from < 0) continue;
    int to = -1;
    for (int64_t m = k + 1; m < utt.nun && to < 0; ++m) to = (int)out[m * PM_COLS + 1];
    if (to < 0) continue;
    const int hi = min(to, T - 1);
    double best = INFINITY;
    int at = PM_NONE;
    for (int t = max(from, 0) + lane; t <= hi; t += 64) {
      const double v = pm_composite(w, total_frames, utt.first + t, mix, parts);
      if (v < best) {
        best = v;
        at = t;
      }
    }
    wave_arg_min(best, at);
    if (lane == 0 && at != PM_NONE) {
      out[k * PM_COLS + 6] = -best;
      out[k * PM_COLS + 7] = (double)at;
    }
  }
}

// the checks every entry makes on the host rows of the utterance table (a table the entry does not take: -1 rows, not looked at)
// -> *most = the frames of the longest utterance
static int check_pm_utts(const char* what, const int64_t* utts_host, int n_utts, int64_t total_frames, int64_t n_phones, int64_t n_units,
                         int64_t* most) {
  TTS_CHECK_ARG(n_utts >= 0 && n_utts <= 65535, "%s: n_utts %d is outside 0 .. 65535", what, n_utts);
  TTS_CHECK_ARG(total_frames >= 0 && total_frames <= INT64_MAX / 256, "%s: total_frames %lld is out of range", what, (long long)total_frames);
  TTS_CHECK_ARG(n_phones <= INT64_MAX / 256 && n_units <= INT64_MAX / 256, "%s: a table's row count is out of range", what);
  TTS_CHECK_ARG(n_utts == 0 || utts_host, "%s: the host copy of the utterance table is missing", what);
  *most = 0;
  for (int u = 0; u < n_utts; ++u) {
    const int64_t* r = utts_host + (int64_t)u * TTS_PROMINENCE_UTT_COLUMNS;
    TTS_CHECK_ARG(r[1] >= 1 && r[1] <= TTS_PROMINENCE_MAX_FRAMES, "%s: utterance %d has %lld frames, an utterance has 1 .. %d", what, u, (long long)r[1],
                  TTS_PROMINENCE_MAX_FRAMES);
    TTS_CHECK_ARG(r[0] >= 0 && r[1] <= total_frames && r[0] <= total_frames - r[1], "%s: utterance %d (frames %lld .. %lld) does not lie inside the %lld frames",
                  what, u, (long long)r[0], (long long)(r[0] + r[1]), (long long)total_frames);
    if (n_phones >= 0)
      TTS_CHECK_ARG(r[2] >= 0 && r[3] >= 0 && r[3] <= n_phones && r[2] <= n_phones - r[3],
                    "%s: utterance %d (phoneme rows %lld .. %lld) does not lie inside the %lld rows", what, u, (long long)r[2], (long long)(r[2] + r[3]),
                    (long long)n_phones);
    if (n_units >= 0)
      TTS_CHECK_ARG(r[4] >= 0 && r[5] >= 0 && r[5] <= n_units && r[4] <= n_units - r[5],
                    "%s: utterance %d (unit rows %lld .. %lld) does not lie inside the %lld rows", what, u, (long long)r[4], (long long)(r[4] + r[5]),
                    (long long)n_units);
    if (r[1] > *most) *most = r[1];
  }
  return TTS_OK;
}

// ascending, disjoint ranges inside [0, T]; `stride` int32 per row, (begin, end) first
static int check_pm_ranges(const char* what, const char* kind, const int32_t* rows_host, int stride, int u, int64_t first, int64_t n, int64_t T) {
  int64_t prev = 0;
  for (int64_t k = 0; k < n; ++k) {
    const int64_t b = rows_host[(first + k) * stride], e = rows_host[(first + k) * stride + 1];
    TTS_CHECK_ARG(b >= 0 && b <= e && e <= T, "%s: utterance %d, %s %lld is frames [%lld, %lld), the utterance has %lld", what, u, kind, (long long)k,
                  (long long)b, (long long)e, (long long)T);
    TTS_CHECK_ARG(b >= prev, "%s: utterance %d, %s %lld begins at frame %lld, before the end of the one in front of it (%lld): the ranges are ascending and disjoint",
                  what, u, kind, (long long)k, (long long)b, (long long)prev);
    prev = e;
  }
  return TTS_OK;
}

int prominence_channels(const float* f0, const float* energy, int64_t total_frames, const int64_t* utts, const int64_t* utts_host, int n_utts,
                        const int32_t* phones, const int32_t* phones_host, int64_t n_phones, double* x, hipStream_t st) {
  int64_t most = 0;
  TTS_CHECK_ARG(n_phones >= 0, "prominence_channels: n_phones is negative");
  if (int rc = check_pm_utts("prominence_channels", utts_host, n_utts, total_frames, n_phones, -1, &most)) return rc;
  TTS_CHECK_ARG(n_phones == 0 || n_utts == 0 || phones_host, "prominence_channels: the host copy of the phoneme table is missing");
  for (int u = 0; u < n_utts; ++u) {
    const int64_t* r = utts_host + (int64_t)u * TTS_PROMINENCE_UTT_COLUMNS;
    if (int rc = check_pm_ranges("prominence_channels", "phoneme", phones_host, 3, u, r[2], r[3], r[1])) return rc;
  }
  if (n_utts == 0) return TTS_OK;
  TTS_CHECK_ARG(f0 && energy && utts && x && (phones || n_phones == 0), "prominence_channels: null pointer");
  hipLaunchKernelGGL(prominence_channels_kernel, dim3((unsigned)n_utts), dim3(PM_THREADS), 0, st, f0, energy, total_frames, utts, phones, n_phones, x);
  return launch_status("prominence_channels");
}

int prominence_cwt(const double* x, int64_t total_frames, const int64_t* utts, const int64_t* utts_host, int n_utts, const double* table, double* w,
                   hipStream_t st) {
  int64_t most = 0;
  if (int rc = check_pm_utts("prominence_cwt", utts_host, n_utts, total_frames, -1, -1, &most)) return rc;
  if (n_utts == 0) return TTS_OK;
  TTS_CHECK_ARG(x && utts && table && w, "prominence_cwt: null pointer");
  const unsigned tiles = (unsigned)((most + PM_THREADS - 1) / PM_THREADS);
  hipLaunchKernelGGL(prominence_cwt_kernel, dim3(tiles, PM_SCALES, (unsigned)n_utts), dim3(PM_THREADS), 0, st, x, total_frames, utts, table, w);
  return launch_status("prominence_cwt");
}

int prominence_units(const double* w, int64_t total_frames, const int64_t* utts, const int64_t* utts_host, int n_utts, const int32_t* units,
                     const int32_t* units_host, int64_t n_units, const double (&weight)[PM_CH], int j_lo, int j_hi, double* rows, double* p,
                     hipStream_t st) {
  static const char* const names[PM_CH] = {"pitch", "energy", "rate"};
  for (int c = 0; c < PM_CH; ++c)
    TTS_CHECK_ARG(weight[c] >= 0.0 && weight[c] < (double)INFINITY, "prominence_units: the %s weight is %g, a weight is finite and not negative", names[c],
                  weight[c]);
  TTS_CHECK_ARG(j_lo >= 0 && j_lo <= j_hi && j_hi < PM_SCALES, "prominence_units: the band [%d, %d] is outside 0 .. %d", j_lo, j_hi, PM_SCALES - 1);
  TTS_CHECK_ARG(n_units >= 0, "prominence_units: n_units is negative");
  int64_t most = 0;
  if (int rc = check_pm_utts("prominence_units", utts_host, n_utts, total_frames, -1, n_units, &most)) return rc;
  TTS_CHECK_ARG(n_units == 0 || n_utts == 0 || units_host, "prominence_units: the host copy of the unit table is missing");
  for (int u = 0; u < n_utts; ++u) {
    const int64_t* r = utts_host + (int64_t)u * TTS_PROMINENCE_UTT_COLUMNS;
    if (int rc = check_pm_ranges("prominence_units", "unit", units_host, 2, u, r[4], r[5], r[1])) return rc;
  }
  if (n_utts == 0) return TTS_OK;
  TTS_CHECK_ARG(w && utts && (units || n_units == 0) && (rows || n_units == 0), "prominence_units: null pointer");
  PmMix mix = {{weight[0], weight[1], weight[2]}, j_lo, j_hi};
  hipLaunchKernelGGL(prominence_units_kernel, dim3((unsigned)n_utts), dim3(PM_THREADS), 0, st, w, total_frames, utts, units, n_units, mix, rows, p);
  return launch_status("prominence_units");
}

}  // namespace tts

extern "C" {
int tts_prominence_max_frames(void) { return TTS_PROMINENCE_MAX_FRAMES; }
int tts_prominence_channels(const float* f0, const float* energy, int64_t total_frames, const int64_t* utts, const int64_t* utts_host,
                            int32_t n_utts, const int32_t* phones, const int32_t* phones_host, int64_t n_phones, double* x,
                            tts_stream_t stream) {
  return tts::prominence_channels(f0, energy, total_frames, utts, utts_host, n_utts, phones, phones_host, n_phones, x, (hipStream_t)stream);
}
int tts_prominence_cwt(const double* x, int64_t total_frames, const int64_t* utts, const int64_t* utts_host, int32_t n_utts,
                       const double* table, double* w, tts_stream_t stream) {
  return tts::prominence_cwt(x, total_frames, utts, utts_host, n_utts, table, w, (hipStream_t)stream);
}
int tts_prominence_units(const double* w, int64_t total_frames, const int64_t* utts, const int64_t* utts_host, int32_t n_utts,
                         const int32_t* units, const int32_t* units_host, int64_t n_units, double weight_pitch, double weight_energy,
                         double weight_rate, int32_t j_lo, int32_t j_hi, double* rows, double* p, tts_stream_t stream) {
  const double weight[3] = {weight_pitch, weight_energy, weight_rate};
  return tts::prominence_units(w, total_frames, utts, utts_host, n_utts, units, units_host, n_units, weight, j_lo, j_hi, rows, p, (hipStream_t)stream);
}
}
