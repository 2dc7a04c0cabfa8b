// Active speech level (ITU-T P.56, method B) of every utterance of a ragged batch, the runs of speech its envelope marks and the
// gain that brings the level to a target (include/toucan_activity.h holds the definition, DESIGN.md section 18 the decisions).
//
//   tts_activity_envelope       passes 1 to 3: start state, sum of squares, peak and the first / last sample at each of the 15
//                               thresholds, per 100 ms segment: three launches
//   tts_activity_level          pass 4: the active counts from those positions, both levels, threshold, gain: one row per utterance
//   tts_activity_runs           pass 5: the envelope against the final threshold, then runs and bounds: two launches
//   tts_activity_tile_segments  segments per workgroup
//
// The envelope (p, q) is a linear recurrence over the samples: passes 1 to 3 over 100 ms segments, the LDS staging and the carry
// of the states (transition T) are segment_scan.h's, and pass 5 walks the segments the same way.  This file holds the envelope's
// step, the ladder, the level and the runs.
//
// The hangover needs no pass over the samples: a segment is no longer than the hangover, so every gap inside it is bridged and
// its first and last sample at a threshold say how many of its samples are active, given the hangover left at its start.  The
// 30 positions of the ladder live in registers (every update fully unrolled).
//
// Batch independence: a segment's chain is the same instructions on the same values whichever lane, workgroup or batch holds it;
// passes 2, 4 and the walk of pass 5 go in index order per utterance.
#include "segment_scan.h"
#include "../../include/toucan_activity.h"

namespace tts {

constexpr int AC_J = TTS_ACTIVITY_THRESHOLDS;
constexpr int AC_POS = 32;  // int32 per slot in pos: 16 (first, last) pairs

// how many thresholds of the ladder q meets: c_j = 2^(j - 15) <= q exactly for j <= (unbiased exponent of q) + 15
__device__ __forceinline__ int ladder_level(double q) {
  const int e = (int)((__double_as_longlong(q) >> 52) & 0x7ff) - 1023;
  return min(max(e + 16, 0), AC_J);
}

enum { AC_ZERO = 0, AC_LADDER = 1, AC_FINAL = 2 };

// AC_ZERO: pass 1, from the zero state, end state -> state[u][k] of every complete segment.  AC_LADDER: pass 3, from state[u][k],
// sq, peak and the positions at the 15 thresholds.  AC_FINAL: pass 5, from state[u][k], the positions at c* -> entry 15 of pos.
template <int MODE>
__global__ __launch_bounds__(SEG_LANES) void envelope_kernel(const float* __restrict__ x, int64_t n_samples, const int64_t* __restrict__ spans,
                                                             int S, const double* __restrict__ table, int64_t max_segments,
                                                             double* __restrict__ state, double* __restrict__ sq, float* __restrict__ peak,
                                                             int32_t* __restrict__ pos, const double* __restrict__ stats) {
  __shared__ float tile[2][SEG_TILE];
  const int u = blockIdx.y, lane = threadIdx.x;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t n_full = sp.count / S;
  const int64_t n_slots = (sp.count + S - 1) / S;
  const int64_t k0 = (int64_t)blockIdx.x * SEG_LANES;
  if (k0 >= (MODE == AC_ZERO ? n_full : n_slots)) return;  // the whole workgroup: before any barrier
  const int64_t k = k0 + lane;
  const float* base = x + sp.begin + k0 * S;
  const int64_t avail = sp.count - k0 * S;  // samples of the utterance from `base` on: > 0
  // samples of this lane's slot: S, fewer in a trailing partial slot, 0 past the utterance
  const int Sk = (int)max((int64_t)0, min((int64_t)S, sp.count - k * S));

  const double g = table[0], h = table[1];
  double p = 0.0, q = 0.0, e = 0.0, cstar = 0.0;
  float pk = 0.0f;
  const int64_t slot = (int64_t)u * max_segments + k;
  if constexpr (MODE != AC_ZERO) {
    if (k < n_slots) {
      p = state[slot * 2 + 0];
      q = state[slot * 2 + 1];
    }
  }
  if constexpr (MODE == AC_FINAL) {
    const double thr_db = stats[(int64_t)u * TTS_ACTIVITY_COLUMNS + 3];
    cstar = thr_db > -INFINITY ? pow(10.0, thr_db / 20.0) : INFINITY;  // an utterance without a level: nothing reaches it
  }

  int first[AC_J], last[AC_J];  // only ever indexed by unrolled constants: registers
#pragma unroll
  for (int j = 0; j < AC_J; ++j) first[j] = last[j] = -1;
  int first_c = -1, last_c = -1;

  walk_segments(tile, base, avail, S, lane, [&](int ts, float xf) {
    const double ax = (double)fabsf(xf);
    p = fma(g, p, h * ax);
    q = fma(g, q, h * p);
    if constexpr (MODE == AC_LADDER) {
      e = fma(ax, ax, e);
      pk = fmaxf(pk, fabsf(xf));
      const int L = ts < Sk ? ladder_level(q) : 0;  // the zeros behind a partial slot are not samples
#pragma unroll
      for (int j = 0; j < AC_J; ++j) {
        const bool at = j < L;
        first[j] = (at && first[j] < 0) ? ts : first[j];
        last[j] = at ? ts : last[j];
      }
    }
    if constexpr (MODE == AC_FINAL) {
      const bool at = ts < Sk && q >= cstar;
      first_c = (at && first_c < 0) ? ts : first_c;
      last_c = at ? ts : last_c;
    }
  });
  if constexpr (MODE == AC_ZERO) {
    if (k < n_full) {
      state[slot * 2 + 0] = p;
      state[slot * 2 + 1] = q;
    }
  }
  if constexpr (MODE == AC_LADDER) {
    if (k < n_slots) {
      sq[slot] = e;
      peak[slot] = pk;
      int32_t* out = pos + slot * AC_POS;
#pragma unroll
      for (int j = 0; j < AC_J; ++j) {
        out[2 * j + 0] = first[j];
        out[2 * j + 1] = last[j];
      }
    }
  }
  if constexpr (MODE == AC_FINAL) {
    if (k < n_slots) {
      pos[slot * AC_POS + 2 * AC_J + 0] = first_c;
      pos[slot * AC_POS + 2 * AC_J + 1] = last_c;
    }
  }
}

// Pass 4, one wavefront per utterance.  Lane j < 15 walks the slots in order with the hangover left at threshold j; then the sum
// of squares in slot order (64 slots loaded by the lanes, added in order by all), the peak, and the levels, the same in every lane.
__global__ __launch_bounds__(64) void level_kernel(const double* __restrict__ sq, const float* __restrict__ peak, const int32_t* __restrict__ pos,
                                                   int64_t n_samples, const int64_t* __restrict__ spans, int S, int64_t max_segments,
                                                   int measure_only, double target, double ceil_lin, int64_t* __restrict__ counts,
                                                   double* __restrict__ sums, double* __restrict__ stats) {
  __shared__ long long a_lds[16];
  const int u = blockIdx.x, lane = threadIdx.x;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t n_slots = (sp.count + S - 1) / S;
  const int64_t I = 2 * (int64_t)S;
  const int64_t row0 = (int64_t)u * max_segments;

  long long a = 0;
  if (lane < AC_J) {
    int64_t r = 0;
    const int32_t* pp = pos + row0 * AC_POS + 2 * lane;
    for (int64_t k = 0; k < n_slots; ++k) {
      const int64_t Sk = min((int64_t)S, sp.count - k * S);
      const int64_t f = pp[k * AC_POS + 0], l = pp[k * AC_POS + 1];
      if (f < 0) {
        a += min(r, Sk);
        r = max((int64_t)0, r - Sk);
      } else {
        const int64_t tail = Sk - 1 - l;
        a += min(r, f) + (l - f + 1) + min(I, tail);
        r = max((int64_t)0, I - tail);
      }
    }
  }
  if (lane < 16) a_lds[lane] = lane < AC_J ? a : 0;
  __syncthreads();

  float pk = 0.0f;
  for (int64_t k = lane; k < n_slots; k += 64) pk = fmaxf(pk, peak[row0 + k]);
  pk = wave_max(pk);
  double total = 0.0;
  for (int64_t k0 = 0; k0 < n_slots; k0 += 64) {
    const int64_t k = k0 + lane;
    const double v = k < n_slots ? sq[row0 + k] : 0.0;
    wave_each_in_order((int)min((int64_t)64, n_slots - k0), [&](int, double vi) { total += vi; }, v);
  }

  const double ninf = -INFINITY, margin = 15.9;
  double active = ninf, longterm = ninf, thr = ninf, activity = 0.0;
  const bool has_level = sp.count > 0 && total > 0.0 && a_lds[0] > 0;
  if (has_level) {
    longterm = 10.0 * log10(total / (double)sp.count);
    double A_prev = 0.0, C_prev = 0.0, D_prev = 0.0;
    bool found = false;
    for (int j = 0; j < AC_J && !found; ++j) {
      if (a_lds[j] <= 0) break;
      const double A = 10.0 * log10(total / (double)a_lds[j]);
      const double C = 20.0 * log10(ldexp(1.0, j - 15));
      const double D = A - C;
      if (D <= margin) {
        found = true;
        if (j == 0) {
          active = A;
          thr = C;
        } else {
          const double w = (D_prev - margin) / (D_prev - D);
          active = A_prev + w * (A - A_prev);
          thr = C_prev + w * (C - C_prev);
        }
      }
      A_prev = A;
      C_prev = C;
      D_prev = D;
    }
    if (!found) {  // every threshold with active samples stands more than the margin under its level: the last of them
      active = A_prev;
      thr = C_prev;
    }
    activity = pow(10.0, (longterm - active) / 10.0);
  }
  float gf = 1.0f;
  if (!measure_only && has_level && pk > 0.0f) gf = ceiling_gain(pow(10.0, (target - active) / 20.0), pk, ceil_lin);
  if (lane < AC_J) counts[(int64_t)u * TTS_ACTIVITY_COUNTS + lane] = a;
  if (lane == 0) {
    sums[2 * u + 0] = total;
    sums[2 * u + 1] = (double)pk;
    double* row = stats + (int64_t)u * TTS_ACTIVITY_COLUMNS;
    row[0] = active;
    row[1] = longterm;
    row[2] = activity;
    row[3] = thr;
    row[4] = 0.0;
    row[5] = 0.0;
    row[6] = (double)gf;
    row[7] = has_level ? active + 20.0 * log10((double)gf) : ninf;
  }
}

// The walk of pass 5, one wavefront per utterance: 64 slots' positions at c* loaded by the lanes, then taken in order (the same in
// every lane; lane 0 writes).  Two samples at c* at most I apart belong to one run.
__global__ __launch_bounds__(64) void runs_kernel(const int32_t* __restrict__ pos, int64_t n_samples, const int64_t* __restrict__ spans, int S,
                                                  int64_t max_segments, int max_runs, int64_t* __restrict__ runs, int64_t* __restrict__ counts,
                                                  double* __restrict__ stats) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const WaveSpan sp = load_span(spans, u, n_samples);
  const int64_t n_slots = (sp.count + S - 1) / S;
  const int64_t I = 2 * (int64_t)S;
  const int32_t* pp = pos + (int64_t)u * max_segments * AC_POS + 2 * AC_J;
  int64_t* out = runs + (int64_t)u * max_runs * 2;
  int64_t n_runs = 0, run_begin = -1, last_at = -1, speech_begin = 0;
  auto close = [&]() {
    if (n_runs == 0) speech_begin = run_begin;
    if (lane == 0 && n_runs < max_runs) {
      out[2 * n_runs + 0] = run_begin;
      out[2 * n_runs + 1] = last_at + 1;
    }
    ++n_runs;
  };
  for (int64_t k0 = 0; k0 < n_slots; k0 += 64) {
    const int64_t k = k0 + lane;
    int f = -1, l = -1;
    if (k < n_slots) {
      f = pp[k * AC_POS + 0];
      l = pp[k * AC_POS + 1];
    }
    wave_each_in_order((int)min((int64_t)64, n_slots - k0), [&](int i, int fi, int li) {
      if (fi < 0) return;
      const int64_t at = (k0 + i) * S + fi;
      if (run_begin < 0) {
        run_begin = at;
      } else if (at - last_at > I) {
        close();
        run_begin = at;
      }
      last_at = (k0 + i) * S + li;
    }, f, l);
  }
  if (run_begin >= 0) close();
  if (lane == 0) {
    counts[(int64_t)u * TTS_ACTIVITY_COUNTS + AC_J] = n_runs;
    stats[(int64_t)u * TTS_ACTIVITY_COLUMNS + 4] = (double)speech_begin;
    stats[(int64_t)u * TTS_ACTIVITY_COLUMNS + 5] = n_runs > 0 ? (double)(last_at + 1) : 0.0;
  }
}

int activity_envelope(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int S, const double* table,
                      int64_t max_segments, double* state, double* sq, float* peak, int32_t* pos, hipStream_t st) {
  if (int rc = check_rate("activity_envelope", S, TTS_ACTIVITY_MIN_RATE, TTS_ACTIVITY_MAX_RATE)) return rc;
  int64_t groups = 0;
  if (int rc = segment_grid("activity_envelope", spans_host, batch, n_samples, S, max_segments, &groups)) return rc;
  if (batch == 0 || groups == 0) return TTS_OK;
  TTS_CHECK_ARG(x && spans && table && state && sq && peak && pos, "activity_envelope: null pointer");
  const dim3 grid((unsigned)groups, (unsigned)batch), block(SEG_LANES);
  hipLaunchKernelGGL((envelope_kernel<AC_ZERO>), grid, block, 0, st, x, n_samples, spans, S, table, max_segments, state, sq, peak, pos,
                     (const double*)nullptr);
  hipLaunchKernelGGL((segment_carry_kernel<2, true>), dim3((unsigned)batch), dim3(64), 0, st, n_samples, spans, S, table + 2, max_segments, state);
  hipLaunchKernelGGL((envelope_kernel<AC_LADDER>), grid, block, 0, st, x, n_samples, spans, S, table, max_segments, state, sq, peak, pos,
                     (const double*)nullptr);
  return launch_status("activity_envelope");
}

int activity_level(const double* sq, const float* peak, const int32_t* pos, int64_t n_samples, const int64_t* spans, int batch, int S,
                   int64_t max_segments, double target, double ceiling, int64_t* counts, double* sums, double* stats, hipStream_t st) {
  if (int rc = check_rate("activity_level", S, TTS_ACTIVITY_MIN_RATE, TTS_ACTIVITY_MAX_RATE)) return rc;
  double ceil_lin = 1.0;
  if (int rc = check_target("activity_level", "dB", batch, n_samples, max_segments, target, ceiling, &ceil_lin)) return rc;
  const bool measure_only = target != target;
  if (batch == 0) return TTS_OK;
  TTS_CHECK_ARG(sq && peak && pos && spans && counts && sums && stats, "activity_level: null pointer");
  hipLaunchKernelGGL(level_kernel, dim3((unsigned)batch), dim3(64), 0, st, sq, peak, pos, n_samples, spans, S, max_segments, measure_only ? 1 : 0,
                     measure_only ? 0.0 : target, ceil_lin, counts, sums, stats);
  return launch_status("activity_level");
}

int activity_runs(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int batch, int S, const double* table,
                  int64_t max_segments, const double* state, int32_t* pos, int max_runs, int64_t* runs, int64_t* counts, double* stats,
                  hipStream_t st) {
  if (int rc = check_rate("activity_runs", S, TTS_ACTIVITY_MIN_RATE, TTS_ACTIVITY_MAX_RATE)) return rc;
  int64_t groups = 0;
  if (int rc = segment_grid("activity_runs", spans_host, batch, n_samples, S, max_segments, &groups)) return rc;
  TTS_CHECK_ARG(max_runs >= 0, "activity_runs: max_runs %d is negative", max_runs);
  if (batch == 0) return TTS_OK;
  TTS_CHECK_ARG(spans && counts && stats && (max_runs == 0 || runs), "activity_runs: null pointer");
  if (groups > 0) {
    TTS_CHECK_ARG(x && table && state && pos, "activity_runs: null pointer");
    const dim3 grid((unsigned)groups, (unsigned)batch), block(SEG_LANES);
    hipLaunchKernelGGL((envelope_kernel<AC_FINAL>), grid, block, 0, st, x, n_samples, spans, S, table, max_segments, const_cast<double*>(state),
                       (double*)nullptr, (float*)nullptr, pos, (const double*)stats);
  }
  hipLaunchKernelGGL(runs_kernel, dim3((unsigned)batch), dim3(64), 0, st, (const int32_t*)pos, n_samples, spans, S, max_segments, max_runs, runs,
                     counts, stats);
  return launch_status("activity_runs");
}

}  // namespace tts

extern "C" {
int tts_activity_tile_segments(void) { return tts::SEG_LANES; }
int tts_activity_envelope(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, int32_t seg_samples,
                          const double* table, int64_t max_segments, double* state, double* sq, float* peak, int32_t* pos, tts_stream_t stream) {
  return tts::activity_envelope(x, n_samples, spans, spans_host, batch, seg_samples, table, max_segments, state, sq, peak, pos,
                                static_cast<hipStream_t>(stream));
}
int tts_activity_level(const double* sq, const float* peak, const int32_t* pos, int64_t n_samples, const int64_t* spans, int32_t batch,
                       int32_t seg_samples, int64_t max_segments, double target_db, double peak_ceiling_dbfs, int64_t* counts, double* sums,
                       double* stats, tts_stream_t stream) {
  return tts::activity_level(sq, peak, pos, n_samples, spans, batch, seg_samples, max_segments, target_db, peak_ceiling_dbfs, counts, sums, stats,
                             static_cast<hipStream_t>(stream));
}
int tts_activity_runs(const float* x, int64_t n_samples, const int64_t* spans, const int64_t* spans_host, int32_t batch, int32_t seg_samples,
                      const double* table, int64_t max_segments, const double* state, int32_t* pos, int32_t max_runs, int64_t* runs,
                      int64_t* counts, double* stats, tts_stream_t stream) {
  return tts::activity_runs(x, n_samples, spans, spans_host, batch, seg_samples, table, max_segments, state, pos, max_runs, runs, counts, stats,
                            static_cast<hipStream_t>(stream));
}
}  // extern "C"
