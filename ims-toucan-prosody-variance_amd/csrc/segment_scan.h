// A linear recurrence over the samples of every utterance of a ragged batch, cut into 100 ms segments: what the loudness meter
// (loudness.hip) and the speech-activity meter (activity.hip) share.  A meter adds its per-sample step and its reduction.
//
// The recurrence is sequential in time but linear, so the state at the end of a segment is M (state at its start) + (end state of
// the same segment run from zero), M the zero-input transition over one segment.  Pass 1 runs every segment from zero, one lane
// per segment; pass 2 (segment_carry_kernel) carries the states along each utterance, s_{k+1} = M s_k + end_k; pass 3 runs every
// segment again from its true start state.  No warm-up is truncated: the result is the sequential one up to fp64 rounding.
//
// A lane's samples are contiguous, so a wavefront reading "sample t of my segment" would touch 64 cache lines per load.  The
// workgroup (one wavefront) therefore stages [SEG_LANES segments] x [SEG_T samples] through LDS (walk_segments): row r is loaded
// by the 64 lanes along the samples (one 256-byte line, dword loads: a segment's first sample has no alignment to speak of), and
// lane r reads row r back.  Rows are SEG_T + 1 dwords apart: lane r reads bank (r + t) mod 32, the lanes of a half-wave all
// different.  The next chunk's loads are issued before the current chunk is worked through and wait in registers meanwhile.
#pragma once
#include <math.h>

#include "common.h"

namespace tts {

constexpr int SEG_LANES = 64;            // segments per workgroup = lanes
constexpr int SEG_T = 64;                // samples of every segment staged at a time
constexpr int SEG_STRIDE = SEG_T + 1;    // dwords between the rows of a tile
constexpr int SEG_TILE = SEG_LANES * SEG_STRIDE;

struct WaveSpan {
  int64_t begin, count;
};

// a row that lies outside the wave counts as an utterance of no samples
__device__ __forceinline__ WaveSpan load_span(const int64_t* __restrict__ spans, int u, int64_t n_samples) {
  WaveSpan s = {spans[2 * u], spans[2 * u + 1]};
  if (s.begin < 0 || s.count < 0 || s.begin > n_samples || s.count > n_samples - s.begin) s.count = 0;
  return s;
}

// step(ts, xf) for sample ts = 0 .. S - 1 of this lane's row, in order: row r of the tile is the S samples from base + r S, `avail`
// (> 0) samples of the utterance lie from `base` on, and what lies past them reads as 0.  The whole workgroup calls it.
template <class Step>
__device__ __forceinline__ void walk_segments(float (&tile)[2][SEG_TILE], const float* __restrict__ base, int64_t avail, int S, int lane,
                                              Step step) {
  const int chunks = (S + SEG_T - 1) / SEG_T;
  float next[SEG_LANES];
  // chunk c of row r: samples r S + c SEG_T + (0 .. SEG_T - 1) from `base`.  fetch() issues all 64 loads, each at an index clamped
  // into the utterance, with 32-bit offsets from the uniform base (a tile spans at most 64 * 19 200 + 64 samples), and uses none
  // of them; park() writes them to LDS, 0 for what lies past the segment or the utterance.  Nothing between the two waits for a
  // load (a select right behind each load had the 64 round trips to memory run one after the other).
  const int lim = (int)min(avail, (int64_t)0x7fffffff);
  auto fetch = [&](int c) {
    const int t = c * SEG_T + lane;
#pragma unroll
    for (int r = 0; r < SEG_LANES; ++r) next[r] = base[min(r * S + t, lim - 1)];
  };
  auto park = [&](int c) {
    const int t = c * SEG_T + lane;
    const bool in_segment = t < S;
    float* col = &tile[c & 1][lane];
#pragma unroll
    for (int r = 0; r < SEG_LANES; ++r) col[r * SEG_STRIDE] = (in_segment && r * S + t < lim) ? next[r] : 0.0f;
  };
  fetch(0);
  park(0);
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    if (c + 1 < chunks) fetch(c + 1);
    const float* row = &tile[c & 1][lane * SEG_STRIDE];
    const int t_end = min(SEG_T, S - c * SEG_T);
    for (int t = 0; t < t_end; ++t) step(c * SEG_T + t, row[t]);
    if (c + 1 < chunks) park(c + 1);  // the other buffer: its last readers passed the barrier of the previous round
    __syncthreads();
  }
}

// Pass 2, one wavefront per utterance: state[u][k] (N doubles) holds end_k and gets s_k, the state at the start of segment k; M is
// the row-major N x N transition.  WITH_PARTIAL: a trailing partial slot gets its start state too (its own end state is never
// stored, so none is loaded).  64 segments at a time: every lane loads its segment's end state, then all lanes walk the same chain
// in order, lane j keeping the s it sees at step j (the in-order walk of wave_ops.h, spelled out here: N values a step).
template <int N, bool WITH_PARTIAL>
__global__ __launch_bounds__(64) void segment_carry_kernel(int64_t n_samples, const int64_t* __restrict__ spans, int S,
                                                           const double* __restrict__ transition, int64_t max_segments,
                                                           double* __restrict__ state) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t n_full = sp.count / S;
  const int64_t n_walk = WITH_PARTIAL ? (sp.count + S - 1) / S : n_full;
  double M[N * N], s[N];
#pragma unroll
  for (int i = 0; i < N * N; ++i) M[i] = transition[i];
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = 0.0;
  double* rows = state + (int64_t)u * max_segments * N;
  for (int64_t k0 = 0; k0 < n_walk; k0 += 64) {
    const int64_t k = k0 + lane;
    double end[N], mine[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      end[i] = k < n_full ? rows[k * N + i] : 0.0;
      mine[i] = 0.0;
    }
    const int steps = (int)min((int64_t)64, n_walk - k0);
    for (int j = 0; j < steps; ++j) {
      double nx[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        nx[i] = __shfl(end[i], j, 64);
        if (lane == j) mine[i] = s[i];
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int c = 0; c < N; ++c) nx[i] = fma(M[N * i + c], s[c], nx[i]);  // fma(M[i][N-1], s[N-1], .. fma(M[i][0], s[0], end_i))
      }
#pragma unroll
      for (int i = 0; i < N; ++i) s[i] = nx[i];
    }
    if (k < n_walk) {
#pragma unroll
      for (int i = 0; i < N; ++i) rows[k * N + i] = mine[i];
    }
  }
}

// What the gating meters share (gate_kernel of loudness.hip, loudness_range_kernel of truepeak.hip), one wavefront per utterance: the
// lanes form z_of(j) of 64 blocks, then every lane takes them in index order (wave_each_in_order) -> the sum and the number of the
// z_j above thr, and the largest z_j of all.
template <class Z>
__device__ __forceinline__ void gated_walk(int64_t n_blocks, int lane, double thr, Z z_of, double& sum, int64_t& kept, double& z_max) {
  sum = 0.0;
  kept = 0;
  z_max = 0.0;
  for (int64_t j0 = 0; j0 < n_blocks; j0 += 64) {
    const int64_t j = j0 + lane;
    double z = 0.0;
    if (j < n_blocks) z = z_of(j);
    wave_each_in_order((int)min((int64_t)64, n_blocks - j0), [&](int, double zi) {
      z_max = fmax(z_max, zi);
      if (zi > thr) {
        sum += zi;
        ++kept;
      }
    }, z);
  }
}

// The fp32 gain nearest to g under which the peak sample pk (> 0) stays at or below ceil_lin.
__device__ __forceinline__ float ceiling_gain(double g, float pk, double ceil_lin) {
  const double lim = ceil_lin / (double)pk;
  const bool limited = lim < g;
  if (limited) g = lim;
  float gf = (float)fmin(g, 3.4028234663852886e38);
  if (limited) {
    // rounding to nearest may have stepped over the ceiling: back off until the fp32 product of the peak sample is under it
    while ((double)gf * (double)pk > ceil_lin || (double)__fmul_rn(pk, gf) > ceil_lin) gf = nextafterf(gf, 0.0f);
  }
  return gf;
}

// the host rows: inside the wave, count >= 0; *most = the largest of what `per` makes of a count
template <class F>
int check_spans(const char* what, const int64_t* spans_host, int batch, int64_t n_samples, F per, int64_t* most) {
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

inline int check_rate(const char* what, int S, int min_rate, int max_rate) {
  TTS_CHECK_ARG(S >= min_rate / 10 && S <= max_rate / 10, "%s: seg_samples %d is outside %d .. %d (a tenth of a sample rate of %d .. %d Hz)", what,
                S, min_rate / 10, max_rate / 10, min_rate, max_rate);
  return TTS_OK;
}

// the checks of a call that reads the wave (after check_rate) -> *groups workgroups per utterance (0: nothing to launch)
inline int segment_grid(const char* what, const int64_t* spans_host, int batch, int64_t n_samples, int S, int64_t max_segments, int64_t* groups) {
  int64_t most = 0;
  if (int rc = check_spans(what, spans_host, batch, n_samples, [S](int64_t c) { return (c + S - 1) / S; }, &most)) return rc;
  TTS_CHECK_ARG(max_segments >= 1 && max_segments >= most, "%s: max_segments %lld is below the %lld segments of the longest utterance", what,
                (long long)max_segments, (long long)most);
  *groups = (most + SEG_LANES - 1) / SEG_LANES;
  TTS_CHECK_ARG(*groups <= 0x7fffffff, "%s: more than 2^31 - 1 workgroups per utterance", what);
  return TTS_OK;
}

// the checks of a call that sets the gain (after check_rate); a NaN target measures only -> *ceil_lin, the ceiling as a factor
inline int check_target(const char* what, const char* unit, int batch, int64_t n_samples, int64_t max_segments, double target, double ceiling,
                        double* ceil_lin) {
  TTS_CHECK_ARG(batch >= 0 && batch <= 65535 && n_samples >= 0 && max_segments >= 1,
                "%s: batch %d is outside 0 .. 65535, n_samples negative or max_segments below 1", what, batch);
  *ceil_lin = 1.0;
  if (target != target) return TTS_OK;
  TTS_CHECK_ARG(isfinite(target) && isfinite(ceiling), "%s: the target %g %s and the peak ceiling %g dBFS must be finite", what, target, unit, ceiling);
  TTS_CHECK_ARG(ceiling <= 0.0, "%s: the peak ceiling %g dBFS is above full scale", what, ceiling);
  *ceil_lin = pow(10.0, ceiling / 20.0);
  return TTS_OK;
}

}  // namespace tts
