// Per-utterance prosody scales and the statistics of what they did (include/toucan_prosody.h).
//
//   tts_prosody_control_v  sequence_ops.hip's prosody_control_kernel with the four scales read per utterance
//   tts_prosody_stats      count, mean and variance of the non-zero pitch / energy entries, frames and phonemes per utterance
//
// Both are bandwidth-trivial (a few kB per utterance): one workgroup per utterance with the scalar kernel's stride loop, so that an
// utterance's result depends on that utterance alone.
#include "common.h"
#include "../../include/toucan_prosody.h"

namespace tts {

namespace {

// ------------------------------------------------------------------------------------------------
// InferenceToucanTTS.py:214-227 + _scale_variance :333-343 with per-utterance scales.
// block_sum and scale_variance are sequence_ops.hip's, token for token: the same sums in the same order, and the same expression
// (v - avg) * scale + avg, which the compiler contracts alike in both files - an utterance equals the scalar kernel's bit for bit
// (tests/test_gpu_prosody_scales.py holds the two against each other).
// ------------------------------------------------------------------------------------------------
__device__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ void scale_variance(float* seq, int r0, int r1, float scale, float* red) {
  // mean over the NON-ZERO entries; every entry (zeros included) is shifted, scaled, shifted back; negatives -> 0
  float s = 0.f, cnt = 0.f;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float v = seq[r];
    if (v != 0.0f) { s += v; cnt += 1.f; }
  }
  s = block_sum(s, red);
  cnt = block_sum(cnt, red);
  const float avg = s / cnt;  // empty selection -> NaN, as torch's mean of an empty tensor
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    float v = seq[r] - avg;
    v = v * scale;
    v = v + avg;
    seq[r] = v < 0.0f ? 0.0f : v;
  }
}

// scales == nullptr: the overrides alone (every scale 1: every scaling step is skipped)
__global__ __launch_bounds__(256) void prosody_control_v_kernel(const float* __restrict__ text, int ld_text, float* pitch, float* energy,
                                                                int* dur, const int* __restrict__ seq_begin,
                                                                const int* __restrict__ seq_end, const float* __restrict__ scales) {
  __shared__ float red[4];
  const int u = blockIdx.x;
  const int r0 = seq_begin[u], r1 = seq_end[u];
  float duration_scale = 1.0f, pitch_scale = 1.0f, energy_scale = 1.0f, pause_scale = 1.0f;
  if (scales) {  // (uniform over the workgroup: the branches below do not diverge around a barrier)
    const float* s = scales + (size_t)u * TTS_PROSODY_SCALES;
    duration_scale = s[0]; pitch_scale = s[1]; energy_scale = s[2]; pause_scale = s[3];
  }
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float* f = text + (size_t)r * ld_text;
    if (f[61] == 0.0f) pitch[r] = 0.0f;
    if (f[15] == 0.0f) energy[r] = 0.0f;
    int d = dur[r];
    if (f[21] == 1.0f) d = 0;
    if (f[16] == 1.0f && pause_scale != 1.0f) d = (int)rintf((float)d * pause_scale);
    if (duration_scale != 1.0f) d = (int)rintf((float)d * duration_scale);
    dur[r] = d;
  }
  __syncthreads();
  if (pitch_scale != 1.0f) scale_variance(pitch, r0, r1, pitch_scale, red);
  if (energy_scale != 1.0f) scale_variance(energy, r0, r1, energy_scale, red);
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

}  // namespace

int prosody_control_v(const float* text, int ld_text, float* pitch, float* energy, int* dur, const int* sb, const int* se, int n_seq,
                      const float* scales, hipStream_t st) {
  TTS_CHECK_ARG(n_seq >= 0, "prosody_control_v: n_seq %d is negative", n_seq);
  if (n_seq == 0) return TTS_OK;
  TTS_CHECK_ARG(text && pitch && energy && dur && sb && se, "prosody_control_v: null pointer");
  TTS_CHECK_ARG(ld_text >= 62, "prosody_control_v: ld_text %d < 62 feature columns", ld_text);
  hipLaunchKernelGGL(prosody_control_v_kernel, dim3(n_seq), dim3(256), 0, st, text, ld_text, pitch, energy, dur, sb, se, scales);
  return launch_status("prosody_control_v");
}

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
int tts_prosody_control_v(const float* text, int32_t ld_text, float* pitch, float* energy, int32_t* dur, const int32_t* seq_begin,
                          const int32_t* seq_end, int32_t n_seq, const float* scales, tts_stream_t stream) {
  return tts::prosody_control_v(text, ld_text, pitch, energy, dur, seq_begin, seq_end, n_seq, scales, static_cast<hipStream_t>(stream));
}
int tts_prosody_stats(const float* pitch, const float* energy, const int32_t* dur, const int32_t* seq_begin, const int32_t* seq_end,
                      int32_t n_seq, float* stats, tts_stream_t stream) {
  return tts::prosody_stats(pitch, energy, dur, seq_begin, seq_end, n_seq, stats, static_cast<hipStream_t>(stream));
}
}  // extern "C"
