// The four prosody knobs - duration, pitch variance, energy variance, pause - and the statistics of what they did
// (include/toucan_tts.h, toucan_prosody.h, toucan_prosody_curves.h, toucan_prosody_fit.h; DESIGN.md sections 14, 15 and 22).
//
//   tts_prosody_control    one set of scales for the whole batch
//   tts_prosody_control_v  four scales per utterance
//   tts_prosody_control_c  per-utterance scales times a per-phoneme curve table, and two additive offsets
//   tts_prosody_stats      count, mean and variance of the non-zero pitch / energy entries, frames and phonemes per utterance
//   tts_prosody_fit        the duration scale, pause scale or span multiplier under which a segment takes a given number of frames
//   tts_prosody_fit_apply  the frames the fit's repair hands out, added behind the control kernel
//
// The three control entries launch ONE kernel: "utterance u equals the scalar call on it alone, bit for bit" compares a kernel with
// itself.  All are bandwidth-trivial (a few kB per utterance): one workgroup per utterance with one stride loop, so that an
// utterance's result depends on that utterance alone, and a thread meets the same rows in every loop.
#include "common.h"
#include "../../include/toucan_prosody_fit.h"

namespace tts {

namespace {

struct ProsodyScales {
  float duration, pitch, energy, pause;
};

// ------------------------------------------------------------------------------------------------
// InferenceToucanTTS.py:214-227 + _scale_variance :333-343.
// Feature columns (Preprocessing/articulatory_features.py:817-901): phoneme 15, silence 16, word-boundary 21, voiced 61.
// ------------------------------------------------------------------------------------------------
// The mean over the NON-ZERO entries of the utterance; every entry (zeros included) is shifted, scaled, shifted back; negatives -> 0.
// Without curves a scale of exactly 1 skips the step, reductions included - (v - avg) * 1 + avg is not v in fp32.  With curves the
// scale of row r is scale * curves[r][col] and the offset curves[r][col + 2] follows: both reductions always run, and a row whose
// effective scale is exactly 1 is not written by the scale step.  scale and curves are uniform over the workgroup: no barrier sits
// under a divergent branch.
__device__ void scale_variance(float* seq, int r0, int r1, float scale, const float* __restrict__ curves, int col, float* red) {
  if (!curves && scale == 1.0f) return;
  float s = 0.f, cnt = 0.f;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float v = seq[r];
    if (v != 0.0f) { s += v; cnt += 1.f; }
  }
  s = block_sum(s, red);
  cnt = block_sum(cnt, red);
  const float avg = s / cnt;  // empty selection -> NaN, as torch's mean of an empty tensor
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float* c = curves ? curves + (size_t)r * TTS_PROSODY_CURVE_COLUMNS : nullptr;
    const float es = c ? scale * c[col] : scale;
    if (es != 1.0f) {
      float v = seq[r] - avg;
      v = v * es;
      v = v + avg;
      seq[r] = v < 0.0f ? 0.0f : v;
    }
    const float o = c ? c[col + 2] : 0.0f;
    if (o != 0.0f) {
      float v = seq[r];
      if (v != 0.0f) {  // unvoiced rows stay unvoiced, non-phoneme rows keep energy 0
        v = v + o;
        seq[r] = v < 0.0f ? 0.0f : v;
      }
    }
  }
}

// The frames of one row: the duration after the overrides, the pause scale and the effective duration scale ed (the caller's one
// fp32 product S.duration * C[r][0], or S.duration alone).  The control kernel and the time-budget solver (prosody_fit_kernel) both
// call it, so the solver counts exactly the frames the control kernel will write.
__device__ __forceinline__ int control_duration(int d, bool boundary, bool silence, float pause, float ed) {
  if (boundary) d = 0;
  if (silence && pause != 1.0f) d = (int)rintf((float)d * pause);
  if (ed != 1.0f) d = (int)rintf((float)d * ed);
  return d;
}

// scales ([n_seq][4]) replaces the batch's four for its utterance when it is there; curves ([rows][5]) may be null as well.
__global__ __launch_bounds__(256) void prosody_control_kernel(const float* __restrict__ text, int ld_text, float* pitch, float* energy,
                                                              int* dur, const int* __restrict__ seq_begin, const int* __restrict__ seq_end,
                                                              ProsodyScales k, const float* __restrict__ scales,
                                                              const float* __restrict__ curves) {
  __shared__ float red[4];
  const int u = blockIdx.x;
  const int r0 = seq_begin[u], r1 = seq_end[u];
  if (scales) {
    const float* s = scales + (size_t)u * TTS_PROSODY_SCALES;
    k.duration = s[0]; k.pitch = s[1]; k.energy = s[2]; k.pause = s[3];
  }
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float* f = text + (size_t)r * ld_text;
    if (f[61] == 0.0f) pitch[r] = 0.0f;
    if (f[15] == 0.0f) energy[r] = 0.0f;
    const float ed = curves ? k.duration * curves[(size_t)r * TTS_PROSODY_CURVE_COLUMNS] : k.duration;
    dur[r] = control_duration(dur[r], f[21] == 1.0f, f[16] == 1.0f, k.pause, ed);
  }
  __syncthreads();
  scale_variance(pitch, r0, r1, k.pitch, curves, 1, red);
  scale_variance(energy, r0, r1, k.energy, curves, 2, red);
}

// ------------------------------------------------------------------------------------------------
// Statistics.  Every sum is an fp64 sum in one fixed order: thread t adds its rows t, t + 256, ... in turn, then block_sum
// (wave_ops.h: butterfly + left fold).
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void prosody_stats_kernel(const float* __restrict__ pitch, const float* __restrict__ energy,
                                                            const int* __restrict__ dur, const int* __restrict__ seq_begin,
                                                            const int* __restrict__ seq_end, float* __restrict__ stats) {
  __shared__ double red[4];
  const int u = blockIdx.x;
  const int r0 = seq_begin[u], r1 = seq_end[u];
  double np = 0.0, sp = 0.0, ne = 0.0, se = 0.0, fr = 0.0;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float p = pitch[r], e = energy[r];
    if (p != 0.0f) { sp += (double)p; np += 1.0; }
    if (e != 0.0f) { se += (double)e; ne += 1.0; }
    fr += (double)dur[r];
  }
  np = block_sum(np, red);
  sp = block_sum(sp, red);
  ne = block_sum(ne, red);
  se = block_sum(se, red);
  fr = block_sum(fr, red);
  const double mp = np > 0.0 ? sp / np : 0.0, me = ne > 0.0 ? se / ne : 0.0;
  double qp = 0.0, qe = 0.0;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float p = pitch[r], e = energy[r];
    if (p != 0.0f) { const double d = (double)p - mp; qp += d * d; }
    if (e != 0.0f) { const double d = (double)e - me; qe += d * d; }
  }
  qp = block_sum(qp, red);
  qe = block_sum(qe, red);
  if (threadIdx.x == 0) {
    float* o = stats + (size_t)u * TTS_PROSODY_STATS;
    o[0] = (float)np; o[1] = (float)mp; o[2] = (float)(np > 0.0 ? qp / np : 0.0);
    o[3] = (float)ne; o[4] = (float)me; o[5] = (float)(ne > 0.0 ? qe / ne : 0.0);
    o[6] = (float)fr; o[7] = (float)(r1 - r0);
  }
}

// ------------------------------------------------------------------------------------------------
// The time budget (include/toucan_prosody_fit.h).  One workgroup per segment; every sum is a sum of 64-bit
// integers, so no result depends on an order.  The sums come back through readfirstlane: the solve's branches and its bisection
// loop are uniform over the workgroup, and no barrier sits under a divergent branch.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long uniform_i64(long long v) {
  const unsigned int lo = __builtin_amdgcn_readfirstlane((int)(unsigned int)(unsigned long long)v);
  const unsigned int hi = __builtin_amdgcn_readfirstlane((int)(unsigned int)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// block_sum of wave_ops.h, the result in scalar registers
__device__ __forceinline__ long long uniform_sum(long long v, long long* red) { return uniform_i64(block_sum(v, red)); }

// Exclusive prefix sum over the 256 threads in thread order, the inclusive one minus the thread's own; *total: the sum of all.
// Every thread calls it.
__device__ __forceinline__ long long exclusive_prefix(long long v, long long* red, long long* total) {
  const long long inc = block_scan_forward(v, red, total, [](long long a, long long b) { return a + b; });
  *total = uniform_i64(*total);
  return inc - v;
}

struct FitRows {
  const float* text;
  int ld_text;
  const int* dur;
  const float* curves;  // the input table or null
  int kind;
  float s_duration, s_pause;  // the utterance's given scales
};

// d'' of row r with the segment's knob at x.  Without a table c is 1 and x * 1 == x: the control kernel's ed, bit for bit.
__device__ __forceinline__ int fit_row(const FitRows& q, int r, float x) {
  const float* f = q.text + (size_t)r * q.ld_text;
  const float c = q.curves ? q.curves[(size_t)r * TTS_PROSODY_CURVE_COLUMNS] : 1.0f;
  float pause = q.s_pause, ed;
  if (q.kind == TTS_FIT_UTT_DURATION) {
    ed = x * c;
  } else if (q.kind == TTS_FIT_UTT_PAUSE) {
    pause = x;
    ed = q.s_duration * c;
  } else {
    ed = q.s_duration * (c * x);
  }
  return control_duration(q.dur[r], f[21] == 1.0f, f[16] == 1.0f, pause, ed);
}

__device__ long long fit_frames(const FitRows& q, int r0, int r1, float x, long long* red) {
  long long s = 0;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) s += fit_row(q, r, x);
  return uniform_sum(s, red);
}

__global__ __launch_bounds__(256) void prosody_fit_fill_kernel(const int* __restrict__ seq_begin, const int* __restrict__ seq_end,
                                                               const float* __restrict__ scales_in, const float* __restrict__ curves_in,
                                                               float* __restrict__ scales_out, float* __restrict__ curves_out,
                                                               int* __restrict__ extra) {
  const int u = blockIdx.x;
  const int r0 = seq_begin[u], r1 = seq_end[u];
  if (threadIdx.x < TTS_PROSODY_SCALES) {
    const size_t i = (size_t)u * TTS_PROSODY_SCALES + threadIdx.x;
    scales_out[i] = scales_in ? scales_in[i] : 1.0f;
  }
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    extra[r] = 0;
    if (curves_out) {
#pragma unroll
      for (int c = 0; c < TTS_PROSODY_CURVE_COLUMNS; ++c) {
        const size_t i = (size_t)r * TTS_PROSODY_CURVE_COLUMNS + c;
        curves_out[i] = curves_in ? curves_in[i] : (c < 3 ? 1.0f : 0.0f);
      }
    }
  }
}

__global__ __launch_bounds__(256) void prosody_fit_kernel(const float* __restrict__ text, int ld_text, const int* __restrict__ dur,
                                                          const int* __restrict__ seg_begin, const int* __restrict__ seg_end,
                                                          const int* __restrict__ seg_seq, const int* __restrict__ seg_kind,
                                                          const float* __restrict__ seg_spec, const float* __restrict__ scales_in,
                                                          const float* __restrict__ curves_in, float* __restrict__ scales_out,
                                                          float* __restrict__ curves_out, int* __restrict__ extra, float* __restrict__ report) {
  __shared__ long long red[4];
  const int s = blockIdx.x;
  const int r0 = seg_begin[s], r1 = seg_end[s], u = seg_seq[s];
  const float* spec = seg_spec + (size_t)s * TTS_FIT_SPEC;
  const long long T = (long long)spec[0];
  const float lo = spec[1], hi = spec[2];
  const bool exact = spec[3] != 0.0f;
  FitRows q = {text, ld_text, dur, curves_in, seg_kind[s], 1.0f, 1.0f};
  if (scales_in) {
    q.s_duration = scales_in[(size_t)u * TTS_PROSODY_SCALES];
    q.s_pause = scales_in[(size_t)u * TTS_PROSODY_SCALES + 3];
  }
  const float given = q.kind == TTS_FIT_UTT_DURATION ? q.s_duration : q.kind == TTS_FIT_UTT_PAUSE ? q.s_pause : 1.0f;
  const long long f_base = fit_frames(q, r0, r1, given, red);
  const long long f_lo = fit_frames(q, r0, r1, lo, red), f_hi = fit_frames(q, r0, r1, hi, red);

  int status, iterations = 0;
  float value = given;
  long long f_value = f_base, missing = 0, extra_rows = 0;
  unsigned int a = __float_as_uint(lo), b = __float_as_uint(hi);  // F(a) < T <= F(b) while the bisection runs
  long long fa = f_lo, fb = f_hi;
  if (f_lo == f_hi) {
    status = TTS_FIT_EMPTY;
  } else if (f_lo > T) {
    status = TTS_FIT_CLAMPED_LOW; value = lo; f_value = f_lo;
  } else if (f_hi < T) {
    status = TTS_FIT_CLAMPED_HIGH; value = hi; f_value = f_hi;
  } else if (f_lo == T) {
    status = TTS_FIT_EXACT; value = lo; f_value = f_lo;
  } else {
    while (b - a > 1) {
      const unsigned int mid = a + (b - a) / 2;
      const long long fm = fit_frames(q, r0, r1, __uint_as_float(mid), red);
      if (fm >= T) { b = mid; fb = fm; }
      else { a = mid; fa = fm; }
      ++iterations;
    }
    if (fb == T) {
      status = TTS_FIT_EXACT; value = __uint_as_float(b); f_value = fb;
    } else if (exact) {
      status = TTS_FIT_REPAIRED; value = __uint_as_float(a); f_value = fa; missing = T - fa;
    } else {
      status = TTS_FIT_NEAREST;
      const bool upper = fb - T < T - fa;
      value = __uint_as_float(upper ? b : a);
      f_value = upper ? fb : fa;
    }
  }

  if (status == TTS_FIT_REPAIRED) {  // `missing` of the n = fb - fa slots, evenly spread, each to the row that owns it
    const long long n = fb - fa;
    const float x0 = __uint_as_float(a), x1 = __uint_as_float(b);
    long long carry = 0, mine = 0;
    for (int base = r0; base < r1; base += 256) {
      const int r = base + threadIdx.x;
      const long long delta = r < r1 ? (long long)fit_row(q, r, x1) - (long long)fit_row(q, r, x0) : 0;
      long long total;
      const long long p = carry + exclusive_prefix(delta, red, &total);
      if (r < r1) {
        const int e = (int)(((p + delta) * missing) / n - (p * missing) / n);
        extra[r] = e;
        mine += e > 0;
      }
      carry += total;
    }
    extra_rows = uniform_sum(mine, red);
  }
  if (status != TTS_FIT_EMPTY) {
    if (q.kind == TTS_FIT_SPAN) {
      if (curves_out)
        for (int r = r0 + threadIdx.x; r < r1; r += 256) {
          const size_t i = (size_t)r * TTS_PROSODY_CURVE_COLUMNS;
          curves_out[i] = (curves_in ? curves_in[i] : 1.0f) * value;
        }
    } else if (threadIdx.x == 0) {
      scales_out[(size_t)u * TTS_PROSODY_SCALES + (q.kind == TTS_FIT_UTT_DURATION ? 0 : 3)] = value;
    }
  }
  if (threadIdx.x == 0) {
    float* o = report + (size_t)s * TTS_FIT_COLUMNS;
    o[0] = (float)T; o[1] = (float)(f_value + missing); o[2] = (float)f_value; o[3] = value;
    o[4] = (float)status; o[5] = (float)iterations; o[6] = (float)extra_rows; o[7] = (float)f_base;
  }
}

__global__ __launch_bounds__(256) void prosody_fit_apply_kernel(int* __restrict__ dur, const int* __restrict__ extra, int rows) {
  const unsigned int r = blockIdx.x * 256u + threadIdx.x;
  if (r < (unsigned int)rows) dur[r] += extra[r];
}

// what: the entry's name in messages.
int prosody_control(const char* what, const float* text, int ld_text, float* pitch, float* energy, int* dur, const int* sb, const int* se,
                    int n_seq, ProsodyScales k, const float* scales, const float* curves, hipStream_t st) {
  if (n_seq == 0) return TTS_OK;
  hipLaunchKernelGGL(prosody_control_kernel, dim3(n_seq), dim3(256), 0, st, text, ld_text, pitch, energy, dur, sb, se, k, scales, curves);
  return launch_status(what);
}

// The argument checks of the _v and _c entries (the scalar entry has none but the launch's own).
int prosody_control_args(const char* what, int n_seq, bool pointers, int ld_text) {
  TTS_CHECK_ARG(n_seq >= 0, "%s: n_seq %d is negative", what, n_seq);
  if (n_seq == 0) return TTS_OK;
  TTS_CHECK_ARG(pointers, "%s: null pointer", what);
  TTS_CHECK_ARG(ld_text >= 62, "%s: ld_text %d < 62 feature columns", what, ld_text);
  return TTS_OK;
}

}  // namespace

int prosody_stats(const float* pitch, const float* energy, const int* dur, const int* sb, const int* se, int n_seq, float* stats,
                  hipStream_t st) {
  TTS_CHECK_ARG(n_seq >= 0, "prosody_stats: n_seq %d is negative", n_seq);
  if (n_seq == 0) return TTS_OK;
  TTS_CHECK_ARG(pitch && energy && dur && sb && se && stats, "prosody_stats: null pointer");
  hipLaunchKernelGGL(prosody_stats_kernel, dim3(n_seq), dim3(256), 0, st, pitch, energy, dur, sb, se, stats);
  return launch_status("prosody_stats");
}

}  // namespace tts

extern "C" {
int tts_prosody_control(const float* text, int32_t ld_text, float* pitch, float* energy, int32_t* dur, const int32_t* seq_begin,
                        const int32_t* seq_end, int32_t n_seq, float duration_scale, float pitch_scale, float energy_scale,
                        float pause_scale, tts_stream_t stream) {
  return tts::prosody_control("prosody_control", text, ld_text, pitch, energy, dur, seq_begin, seq_end, n_seq,
                              {duration_scale, pitch_scale, energy_scale, pause_scale}, nullptr, nullptr, static_cast<hipStream_t>(stream));
}
int tts_prosody_control_v(const float* text, int32_t ld_text, float* pitch, float* energy, int32_t* dur, const int32_t* seq_begin,
                          const int32_t* seq_end, int32_t n_seq, const float* scales, tts_stream_t stream) {
  const int rc = tts::prosody_control_args("prosody_control_v", n_seq, text && pitch && energy && dur && seq_begin && seq_end, ld_text);
  if (rc != TTS_OK) return rc;
  return tts::prosody_control("prosody_control_v", text, ld_text, pitch, energy, dur, seq_begin, seq_end, n_seq, {1.0f, 1.0f, 1.0f, 1.0f},
                              scales, nullptr, static_cast<hipStream_t>(stream));
}
int tts_prosody_control_c(const float* text, int32_t ld_text, float* pitch, float* energy, int32_t* dur, const int32_t* seq_begin,
                          const int32_t* seq_end, int32_t n_seq, const float* scales, const float* curves, tts_stream_t stream) {
  const int rc = tts::prosody_control_args("prosody_control_c", n_seq, text && pitch && energy && dur && seq_begin && seq_end && curves, ld_text);
  if (rc != TTS_OK) return rc;
  return tts::prosody_control("prosody_control_c", text, ld_text, pitch, energy, dur, seq_begin, seq_end, n_seq, {1.0f, 1.0f, 1.0f, 1.0f},
                              scales, curves, static_cast<hipStream_t>(stream));
}
int tts_prosody_stats(const float* pitch, const float* energy, const int32_t* dur, const int32_t* seq_begin, const int32_t* seq_end,
                      int32_t n_seq, float* stats, tts_stream_t stream) {
  return tts::prosody_stats(pitch, energy, dur, seq_begin, seq_end, n_seq, stats, static_cast<hipStream_t>(stream));
}
int tts_prosody_fit(const float* text, int32_t ld_text, const int32_t* dur, const int32_t* seq_begin, const int32_t* seq_end, int32_t n_seq,
                    const int32_t* seg_begin, const int32_t* seg_end, const int32_t* seg_seq, const int32_t* seg_kind, int32_t n_seg,
                    const float* seg_spec, const float* scales_in, const float* curves_in, float* scales_out, float* curves_out,
                    int32_t* extra, float* report, tts_stream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  TTS_CHECK_ARG(n_seq >= 0 && n_seg >= 0, "prosody_fit: n_seq %d or n_seg %d is negative", n_seq, n_seg);
  if (n_seq == 0) {
    TTS_CHECK_ARG(n_seg == 0, "prosody_fit: %d segments and no utterance", n_seg);
    return TTS_OK;
  }
  TTS_CHECK_ARG(seq_begin && seq_end && scales_out && extra, "prosody_fit: null pointer");
  TTS_CHECK_ARG(curves_out || !curves_in, "prosody_fit: a curve table goes in and there is none to write");
  TTS_CHECK_ARG(n_seg == 0 || (text && dur && seg_begin && seg_end && seg_seq && seg_kind && seg_spec && report), "prosody_fit: null pointer");
  TTS_CHECK_ARG(n_seg == 0 || ld_text >= 62, "prosody_fit: ld_text %d < 62 feature columns", ld_text);
  hipLaunchKernelGGL(tts::prosody_fit_fill_kernel, dim3(n_seq), dim3(256), 0, st, seq_begin, seq_end, scales_in, curves_in, scales_out, curves_out,
                     extra);
  if (n_seg > 0)
    hipLaunchKernelGGL(tts::prosody_fit_kernel, dim3(n_seg), dim3(256), 0, st, text, ld_text, dur, seg_begin, seg_end, seg_seq, seg_kind, seg_spec,
                       scales_in, curves_in, scales_out, curves_out, extra, report);
  return tts::launch_status("prosody_fit");
}
int tts_prosody_fit_apply(int32_t* dur, const int32_t* extra, int32_t rows, tts_stream_t stream) {
  TTS_CHECK_ARG(rows >= 0, "prosody_fit_apply: rows %d is negative", rows);
  if (rows == 0) return TTS_OK;
  TTS_CHECK_ARG(dur && extra, "prosody_fit_apply: null pointer");
  hipLaunchKernelGGL(tts::prosody_fit_apply_kernel, dim3((rows - 1) / 256 + 1), dim3(256), 0, static_cast<hipStream_t>(stream), dur, extra, rows);
  return tts::launch_status("prosody_fit_apply");
}
}  // extern "C"
