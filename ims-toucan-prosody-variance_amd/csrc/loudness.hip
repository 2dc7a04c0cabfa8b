// Integrated loudness (ITU-R BS.1770-4) of every utterance of a ragged batch and the gain that brings it to a target
// (include/toucan_loudness.h holds the definition, DESIGN.md section 17 the decisions).
//
//   tts_kweight_energy          K-weighted energy e_k (fp64) and sample peak (fp32) of every 100 ms segment: three launches
//   tts_loudness_gate           blocks, both gates, loudness, gain: one row of eight fp64 per utterance
//   tts_apply_gain              y = x * gain[u], the gain read from that row on the device
//   tts_loudness_tile_segments  segments per workgroup
//
// The K-weighting is a 4th-order recurrence, sequential in time and linear: the three passes over 100 ms segments, the LDS staging
// and the carry of the states are segment_scan.h's.  This file holds the filter's step, the gate and the gain.  The filtered
// signal lives in registers only.
//
// Batch independence: a segment's chain is the same instructions on the same values whichever lane, workgroup or batch holds it;
// pass 2 and the gate add in index order per utterance.
#include "segment_scan.h"
#include "../../include/toucan_loudness.h"

namespace tts {

constexpr int GAIN_THREADS = 256;
constexpr int GAIN_PER_THREAD = 4;
constexpr int GAIN_TILE = GAIN_THREADS * GAIN_PER_THREAD;

// ENERGY = false: pass 1, from the zero state, end state -> state[u][k].  ENERGY = true: pass 3, from state[u][k], e_k and peak.
template <bool ENERGY>
__global__ __launch_bounds__(SEG_LANES) void kweight_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                            int S, const double* __restrict__ table, int64_t max_segments,
                                                            double* __restrict__ state, double* __restrict__ energy, float* __restrict__ peak) {
  __shared__ float tile[2][SEG_TILE];
  const int u = blockIdx.y, lane = threadIdx.x;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t n_full = sp.count / S;
  const int64_t n_slots = (sp.count + S - 1) / S;
  const int64_t k0 = (int64_t)blockIdx.x * SEG_LANES;
  if (k0 >= (ENERGY ? n_slots : n_full)) return;  // the whole workgroup: before any barrier
  const int64_t k = k0 + lane;
  const float* base = x + sp.begin + k0 * S;
  const int64_t avail = sp.count - k0 * S;  // samples of the utterance from `base` on: > 0

  const double b0 = table[0], b1 = table[1], b2 = table[2], a1 = table[3], a2 = table[4], c1 = table[5], c2 = table[6];
  double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, e = 0.0;
  float pk = 0.0f;
  const int64_t slot = (int64_t)u * max_segments + k;
  if constexpr (ENERGY) {
    if (k < n_full) {
      s1 = state[slot * 4 + 0];
      s2 = state[slot * 4 + 1];
      s3 = state[slot * 4 + 2];
      s4 = state[slot * 4 + 3];
    }
  }

  walk_segments(tile, base, avail, S, lane, [&](int, float xf) {
    const double xv = (double)xf;
    const double y1 = fma(b0, xv, s1);
    s1 = fma(-a1, y1, fma(b1, xv, s2));
    s2 = fma(-a2, y1, b2 * xv);
    const double y2 = y1 + s3;
    s3 = fma(-c1, y2, fma(-2.0, y1, s4));
    s4 = fma(-c2, y2, y1);
    if constexpr (ENERGY) {
      e = fma(y2, y2, e);
      pk = fmaxf(pk, fabsf(xf));
    }
  });
  if constexpr (ENERGY) {
    if (k < n_slots) {
      energy[slot] = k < n_full ? e : 0.0;
      peak[slot] = pk;
    }
  } else {
    if (k < n_full) {
      state[slot * 4 + 0] = s1;
      state[slot * 4 + 1] = s2;
      state[slot * 4 + 2] = s3;
      state[slot * 4 + 3] = s4;
    }
  }
}

// One wavefront per utterance.  The z_j of 64 blocks are formed by the lanes, then every lane adds them in index order.
__global__ __launch_bounds__(64) void gate_kernel(const double* __restrict__ energy, const float* __restrict__ peak, int64_t n_samples,
                                                  const int64_t* __restrict__ spans, int S, int64_t max_segments, double z_abs,
                                                  int measure_only, double target, double ceil_lin, double* __restrict__ stats) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t n_full = sp.count / S;
  const int64_t n_slots = (sp.count + S - 1) / S;
  const int64_t n_blocks = n_full >= 4 ? n_full - 3 : 0;
  const double* e = energy + (int64_t)u * max_segments;
  const float* p = peak + (int64_t)u * max_segments;
  const double per = 4.0 * (double)S;

  float pk = 0.0f;
  for (int64_t k = lane; k < n_slots; k += 64) pk = fmaxf(pk, p[k]);
  pk = wave_max(pk);

  // the mean of the z_j above `thr`, in index order; also their number and the largest z_j of all
  auto gated = [&](double thr, double& sum, int64_t& kept, double& z_max) {
    gated_walk(n_blocks, lane, thr, [&](int64_t j) { return (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / per; }, sum, kept, z_max);
  };
  double sum_abs, sum_both = 0.0, z_max, unused;
  int64_t n_abs, n_both = 0;
  gated(z_abs, sum_abs, n_abs, z_max);
  if (n_abs > 0) {
    // past both gates: above the relative threshold and above the absolute one
    const double z_rel = sum_abs / (double)n_abs / 10.0;
    gated(fmax(z_rel, z_abs), sum_both, n_both, unused);
  }
  const double ninf = -INFINITY;
  const double lufs = n_both > 0 ? -0.691 + 10.0 * log10(sum_both / (double)n_both) : ninf;
  const double momentary = (n_blocks > 0 && z_max > 0.0) ? -0.691 + 10.0 * log10(z_max) : ninf;
  float gf = 1.0f;
  if (!measure_only && n_both > 0 && pk > 0.0f) gf = ceiling_gain(pow(10.0, (target - lufs) / 20.0), pk, ceil_lin);
  if (lane == 0) {
    double* row = stats + (int64_t)u * TTS_LOUDNESS_COLUMNS;
    row[0] = lufs;
    row[1] = (double)pk;
    row[2] = (double)n_blocks;
    row[3] = (double)n_abs;
    row[4] = (double)n_both;
    row[5] = momentary;
    row[6] = (double)gf;
    row[7] = lufs + 20.0 * log10((double)gf);
  }
}

// (y may be x: no __restrict__ on either)
__global__ __launch_bounds__(GAIN_THREADS) void apply_gain_kernel(const float* x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                                  const double* __restrict__ stats, float* y) {
  const int u = blockIdx.y;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t i0 = (int64_t)blockIdx.x * GAIN_TILE + threadIdx.x;
  if ((int64_t)blockIdx.x * GAIN_TILE >= sp.count) return;
  const float g = (float)stats[(int64_t)u * TTS_LOUDNESS_COLUMNS + 6];
#pragma unroll
  for (int r = 0; r < GAIN_PER_THREAD; ++r) {
    const int64_t i = i0 + r * GAIN_THREADS;
    if (i < sp.count) y[sp.begin + i] = __fmul_rn(x[sp.begin + i], g);
  }
}

int kweight_energy(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int S, const double* table,
                   int64_t max_segments, double* state, double* energy, float* peak, hipStream_t st) {
  if (int rc = check_rate("kweight_energy", S, TTS_LOUDNESS_MIN_RATE, TTS_LOUDNESS_MAX_RATE)) return rc;
  int64_t groups = 0;
  if (int rc = segment_grid("kweight_energy", spans_host, batch, n_samples, S, max_segments, &groups)) return rc;
  if (batch == 0 || groups == 0) return TTS_OK;
  TTS_CHECK_ARG(x && spans && table && state && energy && peak, "kweight_energy: null pointer");
  const dim3 grid((unsigned)groups, (unsigned)batch), block(SEG_LANES);
  hipLaunchKernelGGL((kweight_kernel<false>), grid, block, 0, st, x, n_samples, spans, S, table, max_segments, state, energy, peak);
  hipLaunchKernelGGL((segment_carry_kernel<4, false>), dim3((unsigned)batch), dim3(64), 0, st, n_samples, spans, S, table + 8, max_segments, state);
  hipLaunchKernelGGL((kweight_kernel<true>), grid, block, 0, st, x, n_samples, spans, S, table, max_segments, state, energy, peak);
  return launch_status("kweight_energy");
}

int loudness_gate(const double* energy, const float* peak, int64_t n_samples, const int64_t* spans, int batch, int S, int64_t max_segments,
                  double target, double ceiling, double* stats, hipStream_t st) {
  if (int rc = check_rate("loudness_gate", S, TTS_LOUDNESS_MIN_RATE, TTS_LOUDNESS_MAX_RATE)) return rc;
  double ceil_lin = 1.0;
  if (int rc = check_target("loudness_gate", "LUFS", batch, n_samples, max_segments, target, ceiling, &ceil_lin)) return rc;
  const bool measure_only = target != target;
  if (batch == 0) return TTS_OK;
  TTS_CHECK_ARG(energy && peak && spans && stats, "loudness_gate: null pointer");
  const double z_abs = pow(10.0, (-70.0 + 0.691) / 10.0);
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)batch), dim3(64), 0, st, energy, peak, n_samples, spans, S, max_segments, z_abs,
                     measure_only ? 1 : 0, measure_only ? 0.0 : target, ceil_lin, stats);
  return launch_status("loudness_gate");
}

int apply_gain(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int64_t max_count,
               const double* stats, float* y, hipStream_t st) {
  int64_t most = 0;
  if (int rc = check_spans("apply_gain", spans_host, batch, n_samples, [](int64_t c) { return c; }, &most)) return rc;
  TTS_CHECK_ARG(max_count >= most, "apply_gain: max_count %lld is below the %lld samples of the longest utterance", (long long)max_count, (long long)most);
  const int64_t tiles = (most + GAIN_TILE - 1) / GAIN_TILE;
  TTS_CHECK_ARG(tiles <= 0x7fffffff, "apply_gain: more than 2^31 - 1 workgroups per utterance");
  if (batch == 0 || tiles == 0) return TTS_OK;
  TTS_CHECK_ARG(x && spans && stats && y, "apply_gain: null pointer");
  hipLaunchKernelGGL(apply_gain_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(GAIN_THREADS), 0, st, x, n_samples, spans, stats, y);
  return launch_status("apply_gain");
}

}  // namespace tts

extern "C" {
int tts_loudness_tile_segments(void) { return tts::SEG_LANES; }
int tts_kweight_energy(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, int32_t seg_samples,
                       const double* table, int64_t max_segments, double* state, double* energy, float* peak, tts_stream_t stream) {
  return tts::kweight_energy(x, n_samples, spans, spans_host, batch, seg_samples, table, max_segments, state, energy, peak,
                             static_cast<hipStream_t>(stream));
}
int tts_loudness_gate(const double* energy, const float* peak, int64_t n_samples, const int64_t* spans, int32_t batch, int32_t seg_samples,
                      int64_t max_segments, double target_lufs, double peak_ceiling_dbfs, double* stats, tts_stream_t stream) {
  return tts::loudness_gate(energy, peak, n_samples, spans, batch, seg_samples, max_segments, target_lufs, peak_ceiling_dbfs, stats,
                            static_cast<hipStream_t>(stream));
}
int tts_apply_gain(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, int64_t max_count,
                   const double* stats, float* y, tts_stream_t stream) {
  return tts::apply_gain(x, n_samples, spans, spans_host, batch, max_count, stats, y, static_cast<hipStream_t>(stream));
}
}  // extern "C"
