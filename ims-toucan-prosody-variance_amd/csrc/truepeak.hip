// True peak (ITU-R BS.1770-4 Annex 2) and loudness range (EBU Tech 3342) of every utterance of a ragged batch, and the gain that
// keeps the true peak under a ceiling (include/toucan_truepeak.h holds the definition, DESIGN.md section 20 the decisions).
//
//   tts_true_peak              max |o| of the F-times oversampled utterance, the oversampled signal in registers only: one launch
//   tts_loudness_range         short-term blocks, both gates, the two order statistics by radix select: one row per utterance
//   tts_truepeak_gain          the gain under the true-peak ceiling, stepped until the reading of the scaled utterance is under it:
//                              tiled rounds over the utterances still stepping, then one workgroup per utterance for the rest
//   tts_limit_true_peak        the look-ahead limiter: peaks between samples, sliding minimum and mean, apply, re-measure, trim
//   tts_truepeak_tile_samples  samples per workgroup
//
// Every oversampled value is resample.hip's chain: K fused multiply-adds in j order from 0 on the table row of its phase.  A
// workgroup stages TP_TILE samples and w either side in LDS, zeros where the utterance has none - the packed wave may hold a
// neighbour there - and the table beside them.
//
// Batch independence: a chain is the same instructions on the same values wherever it runs; maxima do not depend on order; the
// gates add in index order per utterance; the selection counts.
#include "segment_scan.h"
#include "../../include/toucan_loudness.h"
#include "../../include/toucan_truepeak.h"

namespace tts {

constexpr int TP_THREADS = 256;
constexpr int TP_PER_THREAD = 4;
constexpr int TP_TILE = TP_THREADS * TP_PER_THREAD;
constexpr int TP_K = TTS_TRUEPEAK_TAPS;
constexpr int TP_W = TTS_TRUEPEAK_HALF_WIDTH;
constexpr int TP_STAGE = TP_TILE + 2 * TP_W;
constexpr int ST_SEGMENTS = TTS_TRUEPEAK_SHORT_TERM_SEGMENTS;
constexpr int LRA_THREADS = 64;
constexpr int LRA_KEPT = 2048;  // zs_j of an utterance kept in LDS up to this many (3.4 minutes); recomputed per pass beyond

__device__ __forceinline__ int tp_taps(int F) { return F > 1 ? TP_K : 1; }

__device__ __forceinline__ void stage_table(float* tab, const float* __restrict__ table, int F) {
  for (int e = threadIdx.x; e < F * tp_taps(F); e += TP_THREADS) tab[e] = table[e];
}

// acc[p] = o[F i + p], p = 0 .. F - 1, for the sample whose K staged samples start at s: the chains of resample.hip
template <int F>
__device__ __forceinline__ void chains(const float* s, const float* tab, float (&acc)[F]) {
  constexpr int K = F > 1 ? TP_K : 1;
#pragma unroll
  for (int p = 0; p < F; ++p) acc[p] = 0.0f;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float v = s[j];
#pragma unroll
    for (int p = 0; p < F; ++p) acc[p] = __builtin_fmaf(tab[j * F + p], v, acc[p]);
  }
}

// The largest |o| over the samples i0 .. i0 + TP_TILE - 1 of the utterance `sp`, scaled by g, that this thread's four samples give.
// The whole workgroup calls it (two barriers); tab holds the staged table.  with_samples: the scaled samples themselves count too.
template <int F>
__device__ __forceinline__ float tile_peak(const float* __restrict__ x, const WaveSpan sp, int64_t i0, float g, float* stage, const float* tab,
                                           bool with_samples = false) {
  constexpr int W = F > 1 ? TP_W : 0;
  __syncthreads();  // the previous tile's readers are done with `stage`
  for (int e = threadIdx.x; e < TP_TILE + 2 * W; e += TP_THREADS) {
    const int64_t i = i0 - W + e;
    stage[e] = (i >= 0 && i < sp.count) ? __fmul_rn(x[sp.begin + i], g) : 0.0f;
  }
  __syncthreads();
  float m = 0.0f;
#pragma unroll
  for (int r = 0; r < TP_PER_THREAD; ++r) {
    const int t = threadIdx.x + r * TP_THREADS;
    if (i0 + t < sp.count) {
      float acc[F];
      chains<F>(stage + t, tab, acc);
#pragma unroll
      for (int p = 0; p < F; ++p) m = fmaxf(m, fabsf(acc[p]));
      if (with_samples) m = fmaxf(m, fabsf(stage[t + W]));
    }
  }
  return m;
}

template <int F>
__global__ __launch_bounds__(TP_THREADS) void true_peak_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                               const float* __restrict__ table, const double* __restrict__ loudness_stats,
                                                               int with_samples, const int* __restrict__ active,
                                                               float* __restrict__ true_peak) {
  __shared__ float stage[TP_STAGE], tab[4 * TP_K], red[4];
  const int u = blockIdx.y;
  if (active && !active[u]) return;  // the whole workgroup: before any barrier
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t i0 = (int64_t)blockIdx.x * TP_TILE;
  if (i0 >= sp.count) return;  // the whole workgroup: before any barrier
  stage_table(tab, table, F);
  const float g = loudness_stats ? (float)loudness_stats[(int64_t)u * TTS_LOUDNESS_COLUMNS + 6] : 1.0f;
  // (block_max folds the wavefronts left to right where this kernel once paired (0,1),(2,3): the same for m >= 0, never a NaN)
  const float m = block_max(tile_peak<F>(x, sp, i0, g, stage, tab, with_samples != 0), red);
  // |o| >= 0: its bit pattern orders as an unsigned integer the way the value does (a NaN ends above every number and stays)
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned int*>(true_peak) + u, __float_as_uint(m));
}

// The gain under the ceiling, in three parts.  gain_init_kernel sets the first candidate, min(g_l, fl32(C / T)), and whether it
// has to be checked at all.  A round is true_peak_kernel on the utterances still active - the reading of fl32(x g), a tiled launch
// over the whole chip - and gain_step_kernel, which accepts the candidate or steps it.  What is still active after
// TTS_TRUEPEAK_TILED_ROUNDS rounds (a step or two is what happens) goes to truepeak_gain_kernel, one workgroup per utterance,
// which steps on its own until the reading fits.  The candidates and the test are the same in both: so is the result.
__global__ __launch_bounds__(64) void gain_init_kernel(const float* __restrict__ true_peak, int batch, int64_t n_samples,
                                                       const int64_t* __restrict__ spans, double ceil_lin, double* __restrict__ loudness_stats,
                                                       int* __restrict__ steps, int* __restrict__ active) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= batch) return;
  const WaveSpan sp = load_span(spans, u, n_samples);
  double* row = loudness_stats + (int64_t)u * TTS_LOUDNESS_COLUMNS;
  const double lufs = row[0], pk = row[1];
  const float gl = (float)row[6], T = true_peak[u];
  float g = gl;
  int on = 0;
  if (lufs != -INFINITY && pk > 0.0 && T > 0.0f && sp.count > 0) {
    g = fminf(gl, (float)fmin(ceil_lin / (double)T, 3.4028234663852886e38));
    on = (double)g * (double)T * (1.0 + 0x1p-17) > ceil_lin;  // otherwise the reading is under C by the header's bound
  }
  steps[u] = 0;
  active[u] = on;
  if (g != gl) {
    row[6] = (double)g;
    row[7] = lufs + 20.0 * log10((double)g);
  }
}

__global__ __launch_bounds__(64) void gain_step_kernel(const float* __restrict__ reading, int batch, double ceil_lin,
                                                       double* __restrict__ loudness_stats, int* __restrict__ steps, int* __restrict__ active) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= batch || !active[u]) return;
  double* row = loudness_stats + (int64_t)u * TTS_LOUDNESS_COLUMNS;
  const float g = (float)row[6];
  if (!((double)reading[u] > ceil_lin) || steps[u] == TTS_TRUEPEAK_MAX_STEPS || g == 0.0f) {
    active[u] = 0;
    return;
  }
  const float next = nextafterf(g, 0.0f);
  steps[u] += 1;
  row[6] = (double)next;
  row[7] = row[0] + 20.0 * log10((double)next);
}

// One workgroup per utterance that is still active: walks the whole utterance once per candidate gain.
template <int F>
__global__ __launch_bounds__(TP_THREADS) void truepeak_gain_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                                   const float* __restrict__ table, double ceil_lin,
                                                                   double* __restrict__ loudness_stats, int* __restrict__ steps,
                                                                   const int* __restrict__ active) {
  __shared__ float stage[TP_STAGE], tab[4 * TP_K], red[4];
  const int u = blockIdx.x;
  if (!active[u]) return;  // the whole workgroup: before any barrier
  const WaveSpan sp = load_span(spans, u, n_samples);
  double* row = loudness_stats + (int64_t)u * TTS_LOUDNESS_COLUMNS;
  const float first = (float)row[6];
  float g = first;
  int taken = steps[u];
  stage_table(tab, table, F);
  for (;;) {
    float m = 0.0f;
    for (int64_t i0 = 0; i0 < sp.count; i0 += TP_TILE) m = fmaxf(m, tile_peak<F>(x, sp, i0, g, stage, tab));
    m = block_max(m, red);
    if (!((double)m > ceil_lin) || taken == TTS_TRUEPEAK_MAX_STEPS || g == 0.0f) break;
    g = nextafterf(g, 0.0f);
    ++taken;
  }
  if (threadIdx.x == 0 && g != first) {
    steps[u] = taken;
    row[6] = (double)g;
    row[7] = row[0] + 20.0 * log10((double)g);
  }
}

// zs_j of the utterance's energies e: one chain of 30 additions in index order
__device__ __forceinline__ double short_term(const double* __restrict__ e, int64_t j, double per) {
  double s = e[j];
#pragma unroll 6
  for (int k = 1; k < ST_SEGMENTS; ++k) s += e[j + k];
  return s / per;
}

// One wavefront per utterance.  The first pass forms the zs_j and keeps them in LDS where the utterance has at most LRA_KEPT of them;
// a longer one recomputes them wherever they are needed (30 loads that the L1 holds): the same values either way.
__global__ __launch_bounds__(LRA_THREADS) void loudness_range_kernel(const double* __restrict__ energy, const float* __restrict__ peak,
                                                                     const float* __restrict__ true_peak, int64_t n_samples,
                                                                     const int64_t* __restrict__ spans, int S, int64_t max_segments, double z_abs,
                                                                     double* __restrict__ zs, double* __restrict__ stats) {
  __shared__ unsigned int hist[256];
  __shared__ double kept_zs[LRA_KEPT];
  const int u = blockIdx.x, lane = threadIdx.x;
  const WaveSpan sp = load_span(spans, u, n_samples);
  // (no host rows in this call: a count past max_segments slots reads as far as the arrays go)
  const int64_t n_full = min(sp.count / S, max_segments);
  const int64_t n_slots = min((sp.count + S - 1) / S, max_segments);
  const int64_t n_blocks = n_full >= ST_SEGMENTS ? n_full - (ST_SEGMENTS - 1) : 0;
  const double* e = energy + (int64_t)u * max_segments;
  const float* p = peak + (int64_t)u * max_segments;
  const double per = (double)ST_SEGMENTS * (double)S;

  float pk = 0.0f;
  for (int64_t k = lane; k < n_slots; k += LRA_THREADS) pk = fmaxf(pk, p[k]);
  pk = wave_max(pk);

  // the sum of the zs_j above `thr` in index order, their number and the largest zs_j of all (gated_walk of segment_scan.h, as gate_kernel of loudness.hip)
  const bool in_lds = n_blocks <= LRA_KEPT;
  auto z_at = [&](int64_t j) { return in_lds ? kept_zs[j] : short_term(e, j, per); };
  auto gated = [&](double thr, double& sum, int64_t& kept, double& z_max, bool first) {
    auto z_of = [&](int64_t j) {
      const double z = first ? short_term(e, j, per) : z_at(j);
      if (first && in_lds) kept_zs[j] = z;
      if (first && zs) zs[(int64_t)u * max_segments + j] = z;
      return z;
    };
    gated_walk(n_blocks, lane, thr, z_of, sum, kept, z_max);
  };
  double sum_abs, unused_sum, z_max, unused_max, thr = z_abs;
  int64_t n_abs, n_both = 0;
  gated(z_abs, sum_abs, n_abs, z_max, true);
  __syncthreads();  // kept_zs
  if (n_abs > 0) {
    thr = fmax(sum_abs / (double)n_abs / 100.0, z_abs);
    gated(thr, unused_sum, n_both, unused_max, false);
  }

  // The value of 0-based rank `rank` among the zs_j > thr: eight passes over the bit pattern, most significant byte first.  A pass
  // counts the candidates (those that match the bytes fixed so far) by their next byte, and the byte whose running count passes
  // the rank is fixed.  Counts are integers: the outcome is the sort's.
  auto select = [&](int64_t rank) {
    unsigned long long prefix = 0, mask = 0;
#pragma unroll 1  // eight passes over one body, as it was compiled before the scan moved to wave_ops.h (unrolled: 2.4 x the code)
    for (int shift = 56; shift >= 0; shift -= 8) {
      __syncthreads();
      for (int d = lane; d < 256; d += LRA_THREADS) hist[d] = 0;
      __syncthreads();
      for (int64_t j = lane; j < n_blocks; j += LRA_THREADS) {
        const double z = z_at(j);
        const unsigned long long bits = (unsigned long long)__double_as_longlong(z);
        if (z > thr && (bits & mask) == prefix) atomicAdd(&hist[(bits >> shift) & 255], 1u);
      }
      __syncthreads();
      // the bin whose running count passes the rank: four bins per lane, a prefix sum over the lanes, and the one lane whose
      // four bins hold the rank tells the others (walking 255 counts in every lane cost more than everything else here)
      unsigned int c[4], mine = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) mine += c[q] = hist[4 * lane + q];
      const unsigned int upto = wave_scan_forward(mine, [](unsigned int a, unsigned int b) { return a + b; });
      const int64_t before = (int64_t)(upto - mine);
      int d = 4 * lane;
      int64_t left = rank - before;
      const bool here = left >= 0 && rank < (int64_t)upto;
      if (here) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if (left >= (int64_t)c[q] && d == 4 * lane + q) {
            left -= c[q];
            ++d;
          }
        }
      }
      const unsigned long long holder = __ballot(here);
      const int src = holder ? __ffsll((long long)holder) - 1 : 63;  // (one lane, as long as the rank is below the candidates' number)
      d = __shfl(d, src, 64);
      rank = __shfl(left, src, 64);
      prefix |= (unsigned long long)d << shift;
      mask |= 255ull << shift;
    }
    return __longlong_as_double((long long)prefix);
  };
  double low = 0.0, high = 0.0;
  if (n_both > 0) {
    low = select(((n_both - 1) * 10 + 50) / 100);
    high = select(((n_both - 1) * 95 + 50) / 100);
  }
  if (lane == 0) {
    const double ninf = -INFINITY;
    const float T = true_peak[u];
    double* row = stats + (int64_t)u * TTS_DELIVERY_COLUMNS;
    row[0] = (double)T;
    row[1] = T == 0.0f ? ninf : 20.0 * log10((double)T);
    row[2] = (double)pk;
    row[3] = z_max > 0.0 ? -0.691 + 10.0 * log10(z_max) : ninf;
    row[4] = n_both > 0 ? 10.0 * log10(high / low) : 0.0;
    row[5] = n_both > 0 ? -0.691 + 10.0 * log10(low) : ninf;
    row[6] = n_both > 0 ? -0.691 + 10.0 * log10(high) : ninf;
    row[7] = (double)n_both;
    row[8] = (double)n_blocks;
    row[9] = (double)n_abs;
    row[10] = low;
    row[11] = high;
  }
}

// ---- the limiter (steps 1 - 7 of the header)

constexpr int LIM_MAX_W = TTS_LOUDNESS_MAX_RATE / 500;  // 2 ms at the highest rate

// g0 of an utterance from its loudness row: the gain to the target, 1 without a loudness (which also switches the limiter off)
__device__ __forceinline__ float limiter_gain(const double* __restrict__ row, double target) {
  const double lufs = row[0];
  return lufs == -INFINITY ? 1.0f : (float)fmin(pow(10.0, (target - lufs) / 20.0), 3.4028234663852886e38);
}

// Step 2: m[i], the largest |o| strictly between the samples i - 1 and i + 1 of v = fl32(x g0), and |v[i]|.  Sample i's own chains
// give the times i + p / F; the times i - 1 + p / F, p >= 1, are the left neighbour's, passed through LDS (`before`), and for the tile's
// first sample computed by thread 0.  0 for an utterance without a loudness: the limiter leaves it alone.
template <int F>
__global__ __launch_bounds__(TP_THREADS) void limit_peaks_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                                 const float* __restrict__ table, const double* __restrict__ loudness_stats,
                                                                 double target, float* __restrict__ m) {
  constexpr int W = F > 1 ? TP_W : 0;
  __shared__ float stage[TP_STAGE + 1], tab[4 * TP_K], before[TP_TILE + 1];
  const int u = blockIdx.y;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t i0 = (int64_t)blockIdx.x * TP_TILE;
  if (i0 >= sp.count) return;  // the whole workgroup: before any barrier
  const double* row = loudness_stats + (int64_t)u * TTS_LOUDNESS_COLUMNS;
  const bool on = row[0] != -INFINITY;
  const float g0 = limiter_gain(row, target);
  stage_table(tab, table, F);
  // stage[e] = v[i0 - 1 - W + e]: the chains of sample i0 + t start at stage[t + 1], those of sample i0 - 1 at stage[0]
  for (int e = threadIdx.x; e < TP_TILE + 1 + 2 * W; e += TP_THREADS) {
    const int64_t i = i0 - 1 - W + e;
    stage[e] = (i >= 0 && i < sp.count) ? __fmul_rn(x[sp.begin + i], g0) : 0.0f;
  }
  __syncthreads();
  float own[TP_PER_THREAD];
#pragma unroll
  for (int r = 0; r < TP_PER_THREAD; ++r) {
    const int t = threadIdx.x + r * TP_THREADS;
    float a = 0.0f, b = 0.0f;
    if (i0 + t < sp.count) {
      float acc[F];
      chains<F>(stage + t + 1, tab, acc);
#pragma unroll
      for (int p = 1; p < F; ++p) b = fmaxf(b, fabsf(acc[p]));
      a = fmaxf(fmaxf(b, fabsf(acc[0])), fabsf(stage[t + 1 + W]));
    }
    own[r] = a;
    before[t + 1] = b;
  }
  if (threadIdx.x == 0) {
    float b = 0.0f;
    if (i0 >= 1) {
      float acc[F];
      chains<F>(stage, tab, acc);
#pragma unroll
      for (int p = 1; p < F; ++p) b = fmaxf(b, fabsf(acc[p]));
    }
    before[0] = b;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < TP_PER_THREAD; ++r) {
    const int t = threadIdx.x + r * TP_THREADS;
    if (i0 + t < sp.count) m[sp.begin + i0 + t] = on ? fmaxf(own[r], before[t]) : 0.0f;
  }
}

// Steps 3 - 6 for one tile: r = min(1, C / m) of the tile and W either side, h = the minimum of r over the W + 1 samples from each
// on, g = the mean of h over the W + 1 samples up to each - one chain of additions in index order per sample - and
// y' = fl32(fl32(x g0) fl32(g)).  y may be x (a sample is read and written by the same thread): no __restrict__ on either.
__global__ __launch_bounds__(TP_THREADS) void limit_gain_kernel(const float* x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                                const double* __restrict__ loudness_stats, double target, double ceil_lin, int W,
                                                                const float* __restrict__ m, double* __restrict__ g, float* y) {
  __shared__ double r[TP_TILE + 2 * LIM_MAX_W], h[TP_TILE + LIM_MAX_W];
  const int u = blockIdx.y;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t i0 = (int64_t)blockIdx.x * TP_TILE;
  if (i0 >= sp.count) return;  // the whole workgroup: before any barrier
  const float g0 = limiter_gain(loudness_stats + (int64_t)u * TTS_LOUDNESS_COLUMNS, target);
  // r[e] = r of sample i0 - W + e; 1 outside the utterance (neutral in a minimum of values <= 1)
  for (int e = threadIdx.x; e < TP_TILE + 2 * W; e += TP_THREADS) {
    const int64_t j = i0 - W + e;
    double v = 1.0;
    if (j >= 0 && j < sp.count) {
      const float mj = m[sp.begin + j];
      if (mj > 0.0f) v = fmin(1.0, ceil_lin / (double)mj);
    }
    r[e] = v;
  }
  __syncthreads();
  // h[e] = h of sample k = i0 - W + e, also for the W places in front of the utterance, whose windows reach into it
  for (int e = threadIdx.x; e < TP_TILE + W; e += TP_THREADS) {
    double v = r[e];
    for (int d = 1; d <= W; ++d) v = fmin(v, r[e + d]);
    h[e] = v;
  }
  __syncthreads();
  const double width = (double)(W + 1);
#pragma unroll
  for (int q = 0; q < TP_PER_THREAD; ++q) {
    const int t = threadIdx.x + q * TP_THREADS;
    if (i0 + t < sp.count) {
      double s = h[t];  // k = i - W
      for (int d = 1; d <= W; ++d) s += h[t + d];
      const double gi = s / width;
      const int64_t at = sp.begin + i0 + t;
      g[at] = gi;
      y[at] = __fmul_rn(__fmul_rn(x[at], g0), (float)gi);
    }
  }
}

// Step 7, one thread per utterance: the trim t from the larger of the true peak and the sample peak of y', into a row that tts_apply_gain reads (column 6).
__global__ __launch_bounds__(64) void limit_trim_kernel(const double* __restrict__ loudness_stats, int batch, double target, double ceil_lin, int W,
                                                        const float* __restrict__ true_peak, double* __restrict__ rows) {
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= batch) return;
  const double* in = loudness_stats + (int64_t)u * TTS_LOUDNESS_COLUMNS;
  const bool on = in[0] != -INFINITY;
  const float T = true_peak[u];
  float t = 1.0f;
  if (on && (double)T > ceil_lin) t = (float)((ceil_lin / (double)T) * (1.0 - 0x1p-16));
  double* row = rows + (int64_t)u * TTS_LIMITER_COLUMNS;
  row[0] = (double)limiter_gain(in, target);
  row[1] = ceil_lin;
  row[2] = (double)T;
  row[3] = T == 0.0f ? -INFINITY : 20.0 * log10((double)T / ceil_lin);
  row[4] = t != 1.0f ? 1.0 : 0.0;
  row[5] = (double)W;
  row[6] = (double)t;
  row[7] = 20.0 * log10((double)t);
}

static int check_table(const char* what, int factor) {
  TTS_CHECK_ARG(factor == 1 || factor == 2 || factor == 4, "%s: the oversampling factor %d is not 1, 2 or 4", what, factor);
  return TTS_OK;
}

int true_peak(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int64_t max_count, const float* table,
              int factor, const double* loudness_stats, int with_samples, const int* active, float* out, hipStream_t st) {
  if (int rc = check_table("true_peak", factor)) return rc;
  int64_t most = 0;
  if (int rc = check_spans("true_peak", spans_host, batch, n_samples, [](int64_t c) { return c; }, &most)) return rc;
  TTS_CHECK_ARG(max_count >= most, "true_peak: max_count %lld is below the %lld samples of the longest utterance", (long long)max_count, (long long)most);
  const int64_t tiles = (most + TP_TILE - 1) / TP_TILE;
  TTS_CHECK_ARG(tiles <= 0x7fffffff, "true_peak: more than 2^31 - 1 workgroups per utterance");
  if (batch == 0) return TTS_OK;
  TTS_CHECK_ARG((x || most == 0) && spans && table && out, "true_peak: null pointer");  // (a wave of no samples has no address)
  if (hipMemsetAsync(out, 0, (size_t)batch * sizeof(float), st) != hipSuccess) return launch_status("true_peak");
  if (tiles == 0) return TTS_OK;
  const dim3 grid((unsigned)tiles, (unsigned)batch), block(TP_THREADS);
  if (factor == 4) hipLaunchKernelGGL((true_peak_kernel<4>), grid, block, 0, st, x, n_samples, spans, table, loudness_stats, with_samples, active, out);
  else if (factor == 2) hipLaunchKernelGGL((true_peak_kernel<2>), grid, block, 0, st, x, n_samples, spans, table, loudness_stats, with_samples, active, out);
  else hipLaunchKernelGGL((true_peak_kernel<1>), grid, block, 0, st, x, n_samples, spans, table, loudness_stats, with_samples, active, out);
  return launch_status("true_peak");
}

int loudness_range(const double* energy, const float* peak, const float* tp, int64_t n_samples, const int64_t* spans, int batch, int S,
                   int64_t max_segments, double* zs, double* stats, hipStream_t st) {
  if (int rc = check_rate("loudness_range", S, TTS_LOUDNESS_MIN_RATE, TTS_LOUDNESS_MAX_RATE)) return rc;
  TTS_CHECK_ARG(batch >= 0 && batch <= 65535 && n_samples >= 0 && max_segments >= 1,
                "loudness_range: batch %d is outside 0 .. 65535, n_samples negative or max_segments below 1", batch);
  if (batch == 0) return TTS_OK;
  TTS_CHECK_ARG(energy && peak && tp && spans && stats, "loudness_range: null pointer");
  const double z_abs = pow(10.0, (-70.0 + 0.691) / 10.0);
  hipLaunchKernelGGL(loudness_range_kernel, dim3((unsigned)batch), dim3(LRA_THREADS), 0, st, energy, peak, tp, n_samples, spans, S, max_segments,
                     z_abs, zs, stats);
  return launch_status("loudness_range");
}

int truepeak_gain(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, const float* table, int factor,
                  const float* tp, double ceiling, double* loudness_stats, int* steps, int* work, hipStream_t st) {
  if (int rc = check_table("truepeak_gain", factor)) return rc;
  int64_t most = 0;
  if (int rc = check_spans("truepeak_gain", spans_host, batch, n_samples, [](int64_t c) { return c; }, &most)) return rc;
  TTS_CHECK_ARG(isfinite(ceiling), "truepeak_gain: the true-peak ceiling %g dBTP must be finite", ceiling);
  TTS_CHECK_ARG(ceiling <= 0.0, "truepeak_gain: the true-peak ceiling %g dBTP is above full scale", ceiling);
  if (batch == 0) return TTS_OK;
  TTS_CHECK_ARG((x || most == 0) && spans && table && tp && loudness_stats && steps && work, "truepeak_gain: null pointer");
  const double ceil_lin = pow(10.0, ceiling / 20.0);
  int* active = work;
  float* reading = reinterpret_cast<float*>(work + batch);
  const dim3 rows((unsigned)((batch + 63) / 64));
  hipLaunchKernelGGL(gain_init_kernel, rows, dim3(64), 0, st, tp, batch, n_samples, spans, ceil_lin, loudness_stats, steps, active);
  if (int rc = launch_status("truepeak_gain")) return rc;
  for (int round = 0; round < TTS_TRUEPEAK_TILED_ROUNDS && most > 0; ++round) {
    if (int rc = true_peak(x, n_samples, spans, spans_host, batch, most, table, factor, loudness_stats, 0, active, reading, st)) return rc;
    hipLaunchKernelGGL(gain_step_kernel, rows, dim3(64), 0, st, reading, batch, ceil_lin, loudness_stats, steps, active);
  }
  const dim3 grid((unsigned)batch), block(TP_THREADS);
  if (factor == 4) hipLaunchKernelGGL((truepeak_gain_kernel<4>), grid, block, 0, st, x, n_samples, spans, table, ceil_lin, loudness_stats, steps, active);
  else if (factor == 2) hipLaunchKernelGGL((truepeak_gain_kernel<2>), grid, block, 0, st, x, n_samples, spans, table, ceil_lin, loudness_stats, steps, active);
  else hipLaunchKernelGGL((truepeak_gain_kernel<1>), grid, block, 0, st, x, n_samples, spans, table, ceil_lin, loudness_stats, steps, active);
  return launch_status("truepeak_gain");
}


// (loudness.hip)
int apply_gain(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int64_t max_count,
               const double* stats, float* y, hipStream_t st);

int limit_true_peak(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int64_t max_count, int S,
                    const float* table, int factor, const double* loudness_stats, double target, double ceiling, double tp_ceiling, float* m,
                    double* g, float* tp, double* rows, float* y, hipStream_t st) {
  if (int rc = check_rate("limit_true_peak", S, TTS_LOUDNESS_MIN_RATE, TTS_LOUDNESS_MAX_RATE)) return rc;
  if (int rc = check_table("limit_true_peak", factor)) return rc;
  int64_t most = 0;
  if (int rc = check_spans("limit_true_peak", spans_host, batch, n_samples, [](int64_t c) { return c; }, &most)) return rc;
  TTS_CHECK_ARG(max_count >= most, "limit_true_peak: max_count %lld is below the %lld samples of the longest utterance", (long long)max_count,
                (long long)most);
  TTS_CHECK_ARG(isfinite(target) && isfinite(ceiling) && isfinite(tp_ceiling),
                "limit_true_peak: the target %g LUFS, the peak ceiling %g dBFS and the true-peak ceiling %g dBTP must be finite", target, ceiling, tp_ceiling);
  TTS_CHECK_ARG(ceiling <= 0.0 && tp_ceiling <= 0.0, "limit_true_peak: the ceilings %g dBFS and %g dBTP: one is above full scale", ceiling, tp_ceiling);
  const int64_t tiles = (most + TP_TILE - 1) / TP_TILE;
  TTS_CHECK_ARG(tiles <= 0x7fffffff, "limit_true_peak: more than 2^31 - 1 workgroups per utterance");
  if (batch == 0) return TTS_OK;
  TTS_CHECK_ARG(((x && m && g && y) || most == 0) && spans && table && loudness_stats && tp && rows, "limit_true_peak: null pointer");
  const int W = S / 50;  // fs / 500
  const double ceil_lin = pow(10.0, fmin(ceiling, tp_ceiling) / 20.0);
  if (tiles > 0) {
    const dim3 grid((unsigned)tiles, (unsigned)batch), block(TP_THREADS);
    if (factor == 4) hipLaunchKernelGGL((limit_peaks_kernel<4>), grid, block, 0, st, x, n_samples, spans, table, loudness_stats, target, m);
    else if (factor == 2) hipLaunchKernelGGL((limit_peaks_kernel<2>), grid, block, 0, st, x, n_samples, spans, table, loudness_stats, target, m);
    else hipLaunchKernelGGL((limit_peaks_kernel<1>), grid, block, 0, st, x, n_samples, spans, table, loudness_stats, target, m);
    hipLaunchKernelGGL(limit_gain_kernel, grid, block, 0, st, x, n_samples, spans, loudness_stats, target, ceil_lin, W, m, g, y);
    if (int rc = launch_status("limit_true_peak")) return rc;
  }
  if (int rc = true_peak(y, n_samples, spans, spans_host, batch, max_count, table, factor, nullptr, 1, nullptr, tp, st)) return rc;
  hipLaunchKernelGGL(limit_trim_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, st, loudness_stats, batch, target, ceil_lin, W, tp, rows);
  if (int rc = launch_status("limit_true_peak")) return rc;
  return apply_gain(y, n_samples, spans, spans_host, batch, max_count, rows, y, st);
}

}  // namespace tts

extern "C" {
int tts_truepeak_tile_samples(void) { return tts::TP_TILE; }
int tts_true_peak(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, int64_t max_count,
                  const float* table, int32_t factor, const double* loudness_stats, float* true_peak, tts_stream_t stream) {
  return tts::true_peak(x, n_samples, spans, spans_host, batch, max_count, table, factor, loudness_stats, 0, nullptr, true_peak, static_cast<hipStream_t>(stream));
}
int tts_loudness_range(const double* energy, const float* peak, const float* true_peak, int64_t n_samples, const int64_t* spans, int32_t batch,
                       int32_t seg_samples, int64_t max_segments, double* zs, double* stats, tts_stream_t stream) {
  return tts::loudness_range(energy, peak, true_peak, n_samples, spans, batch, seg_samples, max_segments, zs, stats, static_cast<hipStream_t>(stream));
}
int tts_truepeak_gain(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, const float* table,
                      int32_t factor, const float* true_peak, double true_peak_ceiling_dbtp, double* loudness_stats, int32_t* steps,
                      int32_t* work, tts_stream_t stream) {
  return tts::truepeak_gain(x, n_samples, spans, spans_host, batch, table, factor, true_peak, true_peak_ceiling_dbtp, loudness_stats, steps, work,
                            static_cast<hipStream_t>(stream));
}
int tts_limit_true_peak(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, int64_t max_count,
                        int32_t seg_samples, const float* table, int32_t factor, const double* loudness_stats, double target_lufs,
                        double peak_ceiling_dbfs, double true_peak_ceiling_dbtp, float* m, double* g, float* true_peak, double* limiter_stats, float* y,
                        tts_stream_t stream) {
  return tts::limit_true_peak(x, n_samples, spans, spans_host, batch, max_count, seg_samples, table, factor, loudness_stats, target_lufs,
                              peak_ceiling_dbfs, true_peak_ceiling_dbtp, m, g, true_peak, limiter_stats, y, static_cast<hipStream_t>(stream));
}
}  // extern "C"
