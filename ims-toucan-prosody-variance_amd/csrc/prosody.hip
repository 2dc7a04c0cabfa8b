// The four prosody knobs - duration, pitch variance, energy variance, pause - and the statistics of what they did
// (include/toucan_tts.h, toucan_prosody.h, toucan_prosody_curves.h; DESIGN.md sections 14 and 15).
//
//   tts_prosody_control    one set of scales for the whole batch
//   tts_prosody_control_v  four scales per utterance
//   tts_prosody_control_c  per-utterance scales times a per-phoneme curve table, and two additive offsets
//   tts_prosody_stats      count, mean and variance of the non-zero pitch / energy entries, frames and phonemes per utterance
//
// The three control entries launch ONE kernel: "utterance u equals the scalar call on it alone, bit for bit" compares a kernel with
// itself.  All are bandwidth-trivial (a few kB per utterance): one workgroup per utterance with one stride loop, so that an
// utterance's result depends on that utterance alone, and a thread meets the same rows in every loop.
#include "common.h"
#include "../../include/toucan_prosody_curves.h"

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
    int d = dur[r];
    if (f[21] == 1.0f) d = 0;
    if (f[16] == 1.0f && k.pause != 1.0f) d = (int)rintf((float)d * k.pause);
    const float ed = curves ? k.duration * curves[(size_t)r * TTS_PROSODY_CURVE_COLUMNS] : k.duration;
    if (ed != 1.0f) d = (int)rintf((float)d * ed);
    dur[r] = d;
  }
  __syncthreads();
  scale_variance(pitch, r0, r1, k.pitch, curves, 1, red);
  scale_variance(energy, r0, r1, k.energy, curves, 2, red);
}

// ------------------------------------------------------------------------------------------------
// Statistics.  Every sum is an fp64 sum in one fixed order: thread t adds its rows t, t + 256, ... in turn, the 64 lanes of a
// wavefront are folded by the xor butterfly (32, 16, ... 1), the four wavefronts are added 0 + 1 + 2 + 3.
// ------------------------------------------------------------------------------------------------
__device__ double block_sum_f64(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

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
  np = block_sum_f64(np, red);
  sp = block_sum_f64(sp, red);
  ne = block_sum_f64(ne, red);
  se = block_sum_f64(se, red);
  fr = block_sum_f64(fr, red);
  const double mp = np > 0.0 ? sp / np : 0.0, me = ne > 0.0 ? se / ne : 0.0;
  double qp = 0.0, qe = 0.0;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float p = pitch[r], e = energy[r];
    if (p != 0.0f) { const double d = (double)p - mp; qp += d * d; }
    if (e != 0.0f) { const double d = (double)e - me; qe += d * d; }
  }
  qp = block_sum_f64(qp, red);
  qe = block_sum_f64(qe, red);
  if (threadIdx.x == 0) {
    float* o = stats + (size_t)u * TTS_PROSODY_STATS;
    o[0] = (float)np; o[1] = (float)mp; o[2] = (float)(np > 0.0 ? qp / np : 0.0);
    o[3] = (float)ne; o[4] = (float)me; o[5] = (float)(ne > 0.0 ? qe / ne : 0.0);
    o[6] = (float)fr; o[7] = (float)(r1 - r0);
  }
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
}  // extern "C"
