// Integrated loudness (ITU-R BS.1770-4) of every utterance of a ragged batch and the gain that brings it to a target
// (include/toucan_loudness.h holds the definition, DESIGN.md section 17 the decisions).
//
//   tts_kweight_energy          K-weighted energy e_k (fp64) and sample peak (fp32) of every 100 ms segment: three launches
//   tts_loudness_gate           blocks, both gates, loudness, gain: one row of eight fp64 per utterance
//   tts_apply_gain              y = x * gain[u], the gain read from that row on the device
//   tts_loudness_tile_segments  segments per workgroup
//
// The K-weighting is a 4th-order recurrence, sequential in time.  It is linear, so the state at the end of a segment is
// M (state at its start) + (end state of the same segment run from zero), M the zero-input transition over one segment.  Pass 1
// runs every segment from zero, one lane per segment; pass 2 carries the states along each utterance, s_{k+1} = M s_k + end_k;
// pass 3 runs every segment again from its true start state and sums the squares.  No warm-up is truncated: the result is the
// sequential one up to fp64 rounding.  The filtered signal lives in registers only.
//
// A lane's samples are contiguous, so a wavefront reading "sample t of my segment" would touch 64 cache lines per load.  The
// workgroup (one wavefront) therefore stages [LD_SEGS segments] x [LD_T samples] through LDS: row r is loaded by the 64 lanes
// along the samples (one 256-byte line, dword loads: a segment's first sample has no alignment to speak of), and lane r reads
// row r back.  Rows are LD_T + 1 dwords apart: lane r reads bank (r + t) mod 32, the lanes of a half-wave all different.  The
// next chunk's loads are issued before the current chunk is filtered and wait in registers meanwhile.
//
// Batch independence: a segment's chain is the same instructions on the same values whichever lane, workgroup or batch holds it;
// pass 2 and the gate add in index order per utterance.
#include <math.h>

#include "common.h"
#include "../../include/toucan_loudness.h"

namespace tts {

constexpr int LD_SEGS = 64;             // segments per workgroup = lanes
constexpr int LD_T = 64;                // samples of every segment staged at a time
constexpr int LD_STRIDE = LD_T + 1;     // dwords between the rows of a tile
constexpr int GAIN_THREADS = 256;
constexpr int GAIN_PER_THREAD = 4;
constexpr int GAIN_TILE = GAIN_THREADS * GAIN_PER_THREAD;

struct LoudSpan {
  int64_t begin, count;
};

// a row that does not lie inside the wave counts as an utterance of no samples
__device__ __forceinline__ LoudSpan load_span(const int64_t* __restrict__ spans, int u, int64_t n_samples) {
  LoudSpan s = {spans[2 * u], spans[2 * u + 1]};
  if (s.begin < 0 || s.count < 0 || s.begin > n_samples || s.count > n_samples - s.begin) s.count = 0;
  return s;
}

// ENERGY = false: pass 1, from the zero state, end state -> state[u][k].  ENERGY = true: pass 3, from state[u][k], e_k and peak.
template <bool ENERGY>
__global__ __launch_bounds__(LD_SEGS) void kweight_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                          int S, const double* __restrict__ table, int64_t max_segments,
                                                          double* __restrict__ state, double* __restrict__ energy, float* __restrict__ peak) {
  __shared__ float tile[2][LD_SEGS * LD_STRIDE];
  const int u = blockIdx.y, lane = threadIdx.x;
  const LoudSpan sp = load_span(spans, u, n_samples);
  const int64_t n_full = sp.count / S;
  const int64_t n_slots = (sp.count + S - 1) / S;
  const int64_t k0 = (int64_t)blockIdx.x * LD_SEGS;
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

  const int chunks = (S + LD_T - 1) / LD_T;
  float next[LD_SEGS];
  // chunk c of row r: samples r S + c LD_T + (0 .. LD_T - 1) from `base`.  fetch() issues all 64 loads, each at an index clamped
  // into the utterance, with 32-bit offsets from the uniform base (a tile spans at most 64 * 19 200 + 64 samples), and uses none
  // of them; park() writes them to LDS, 0 for what lies past the segment or the utterance.  Nothing between the two waits for a
  // load (a select right behind each load had the 64 round trips to memory run one after the other).
  const int lim = (int)min(avail, (int64_t)0x7fffffff);
  auto fetch = [&](int c) {
    const int t = c * LD_T + lane;
#pragma unroll
    for (int r = 0; r < LD_SEGS; ++r) next[r] = base[min(r * S + t, lim - 1)];
  };
  auto park = [&](int c) {
    const int t = c * LD_T + lane;
    const bool in_segment = t < S;
    float* col = &tile[c & 1][lane];
#pragma unroll
    for (int r = 0; r < LD_SEGS; ++r) col[r * LD_STRIDE] = (in_segment && r * S + t < lim) ? next[r] : 0.0f;
  };
  fetch(0);
  park(0);
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    if (c + 1 < chunks) fetch(c + 1);
    const float* row = &tile[c & 1][lane * LD_STRIDE];
    const int t_end = min(LD_T, S - c * LD_T);
    for (int t = 0; t < t_end; ++t) {
      const float xf = row[t];
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
    }
    if (c + 1 < chunks) park(c + 1);  // the other buffer: its last readers passed the barrier of the previous round
    __syncthreads();
  }
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

// Pass 2, one wavefront per utterance: state[u][k] holds end_k and gets s_k, the state at the start of segment k.  64 segments at
// a time: every lane loads its segment's end state, then all lanes walk the same chain in order, lane j keeping the s it sees at
// step j.
__global__ __launch_bounds__(64) void carry_kernel(int64_t n_samples, const int64_t* __restrict__ spans, int S,
                                                   const double* __restrict__ table, int64_t max_segments, double* __restrict__ state) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const LoudSpan sp = load_span(spans, u, n_samples);
  const int64_t n_full = sp.count / S;
  double M[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) M[i] = table[8 + i];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  double* rows = state + (int64_t)u * max_segments * 4;
  for (int64_t k0 = 0; k0 < n_full; k0 += 64) {
    const int64_t k = k0 + lane;
    double end[4] = {0.0, 0.0, 0.0, 0.0}, mine[4] = {0.0, 0.0, 0.0, 0.0};
    if (k < n_full) {
#pragma unroll
      for (int i = 0; i < 4; ++i) end[i] = rows[k * 4 + i];
    }
    const int steps = (int)min((int64_t)64, n_full - k0);
    for (int j = 0; j < steps; ++j) {
      double ej[4], nx[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ej[i] = __shfl(end[i], j, 64);
      if (lane == j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) mine[i] = s[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        nx[i] = fma(M[4 * i + 3], s[3], fma(M[4 * i + 2], s[2], fma(M[4 * i + 1], s[1], fma(M[4 * i + 0], s[0], ej[i]))));
#pragma unroll
      for (int i = 0; i < 4; ++i) s[i] = nx[i];
    }
    if (k < n_full) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rows[k * 4 + i] = mine[i];
    }
  }
}

// One wavefront per utterance.  The z_j of 64 blocks are formed by the lanes, then every lane adds them in index order.
__global__ __launch_bounds__(64) void gate_kernel(const double* __restrict__ energy, const float* __restrict__ peak, int64_t n_samples,
                                                  const int64_t* __restrict__ spans, int S, int64_t max_segments, double z_abs,
                                                  int measure_only, double target, double ceil_lin, double* __restrict__ stats) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const LoudSpan sp = load_span(spans, u, n_samples);
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
    sum = 0.0;
    kept = 0;
    z_max = 0.0;
    for (int64_t j0 = 0; j0 < n_blocks; j0 += 64) {
      const int64_t j = j0 + lane;
      double z = 0.0;
      if (j < n_blocks) z = (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / per;
      const int steps = (int)min((int64_t)64, n_blocks - j0);
      for (int i = 0; i < steps; ++i) {
        const double zi = __shfl(z, i, 64);
        z_max = fmax(z_max, zi);
        if (zi > thr) {
          sum += zi;
          ++kept;
        }
      }
    }
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
  if (!measure_only && n_both > 0 && pk > 0.0f) {
    double g = pow(10.0, (target - lufs) / 20.0);
    const double lim = ceil_lin / (double)pk;
    const bool limited = lim < g;
    if (limited) g = lim;
    gf = (float)fmin(g, 3.4028234663852886e38);
    if (limited) {
      // rounding to nearest may have stepped over the ceiling: back off until the fp32 product of the peak sample is under it
      while ((double)gf * (double)pk > ceil_lin || (double)__fmul_rn(pk, gf) > ceil_lin) gf = nextafterf(gf, 0.0f);
    }
  }
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
  const LoudSpan sp = load_span(spans, u, n_samples);
  const int64_t i0 = (int64_t)blockIdx.x * GAIN_TILE + threadIdx.x;
  if ((int64_t)blockIdx.x * GAIN_TILE >= sp.count) return;
  const float g = (float)stats[(int64_t)u * TTS_LOUDNESS_COLUMNS + 6];
#pragma unroll
  for (int r = 0; r < GAIN_PER_THREAD; ++r) {
    const int64_t i = i0 + r * GAIN_THREADS;
    if (i < sp.count) y[sp.begin + i] = __fmul_rn(x[sp.begin + i], g);
  }
}

// the host rows: inside the wave, count >= 0; *most = the largest of what `per` makes of a count
template <class F>
static int check_spans(const char* what, const int64_t* spans_host, int batch, int64_t n_samples, F per, int64_t* most) {
  TTS_CHECK_ARG(batch >= 0 && batch <= 65535, "%s: batch %d is outside 0 .. 65535", what, batch);
  TTS_CHECK_ARG(n_samples >= 0, "%s: n_samples is negative", what);
  TTS_CHECK_ARG(batch == 0 || spans_host, "%s: the host copy of the spans is missing", what);
  *most = 0;
  for (int u = 0; u < batch; ++u) {
    const int64_t b = spans_host[2 * u], c = spans_host[2 * u + 1];
    TTS_CHECK_ARG(c >= 0, "%s: utterance %d has the negative sample count %lld", what, u, (long long)c);
    TTS_CHECK_ARG(b >= 0 && b <= n_samples && c <= n_samples - b, "%s: utterance %d (samples %lld .. %lld) does not lie inside the wave of %lld samples",
                  what, u, (long long)b, (long long)(b + c), (long long)n_samples);
    const int64_t v = per(c);
    if (v > *most) *most = v;
  }
  return TTS_OK;
}

static int check_rate(const char* what, int S) {
  TTS_CHECK_ARG(S >= TTS_LOUDNESS_MIN_RATE / 10 && S <= TTS_LOUDNESS_MAX_RATE / 10,
                "%s: seg_samples %d is outside %d .. %d (a tenth of a sample rate of %d .. %d Hz)", what, S, TTS_LOUDNESS_MIN_RATE / 10,
                TTS_LOUDNESS_MAX_RATE / 10, TTS_LOUDNESS_MIN_RATE, TTS_LOUDNESS_MAX_RATE);
  return TTS_OK;
}

int kweight_energy(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int S, const double* table,
                   int64_t max_segments, double* state, double* energy, float* peak, hipStream_t st) {
  if (int rc = check_rate("kweight_energy", S)) return rc;
  int64_t most = 0;
  if (int rc = check_spans("kweight_energy", spans_host, batch, n_samples, [S](int64_t c) { return (c + S - 1) / S; }, &most)) return rc;
  TTS_CHECK_ARG(max_segments >= 1 && max_segments >= most, "kweight_energy: max_segments %lld is below the %lld segments of the longest utterance",
                (long long)max_segments, (long long)most);
  const int64_t groups = (most + LD_SEGS - 1) / LD_SEGS;
  TTS_CHECK_ARG(groups <= 0x7fffffff, "kweight_energy: more than 2^31 - 1 workgroups per utterance");
  if (batch == 0 || groups == 0) return TTS_OK;
  TTS_CHECK_ARG(x && spans && table && state && energy && peak, "kweight_energy: null pointer");
  const dim3 grid((unsigned)groups, (unsigned)batch), block(LD_SEGS);
  hipLaunchKernelGGL((kweight_kernel<false>), grid, block, 0, st, x, n_samples, spans, S, table, max_segments, state, energy, peak);
  hipLaunchKernelGGL(carry_kernel, dim3((unsigned)batch), dim3(64), 0, st, n_samples, spans, S, table, max_segments, state);
  hipLaunchKernelGGL((kweight_kernel<true>), grid, block, 0, st, x, n_samples, spans, S, table, max_segments, state, energy, peak);
  return launch_status("kweight_energy");
}

int loudness_gate(const double* energy, const float* peak, int64_t n_samples, const int64_t* spans, int batch, int S, int64_t max_segments,
                  double target, double ceiling, double* stats, hipStream_t st) {
  if (int rc = check_rate("loudness_gate", S)) return rc;
  TTS_CHECK_ARG(batch >= 0 && batch <= 65535 && n_samples >= 0 && max_segments >= 1, "loudness_gate: batch %d is outside 0 .. 65535, n_samples negative or max_segments below 1", batch);
  const bool measure_only = target != target;
  if (!measure_only) {
    TTS_CHECK_ARG(isfinite(target) && isfinite(ceiling), "loudness_gate: the target %g LUFS and the peak ceiling %g dBFS must be finite", target, ceiling);
    TTS_CHECK_ARG(ceiling <= 0.0, "loudness_gate: the peak ceiling %g dBFS is above full scale", ceiling);
  }
  if (batch == 0) return TTS_OK;
  TTS_CHECK_ARG(energy && peak && spans && stats, "loudness_gate: null pointer");
  const double z_abs = pow(10.0, (-70.0 + 0.691) / 10.0);
  const double ceil_lin = measure_only ? 1.0 : pow(10.0, ceiling / 20.0);
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
int tts_loudness_tile_segments(void) { return tts::LD_SEGS; }
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
