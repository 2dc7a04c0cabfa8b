// Per-phoneme prosody curves (include/toucan_prosody_curves.h).
//
//   tts_prosody_control_c  prosody.hip's prosody_control_v_kernel with every scale multiplied, row by row, by a column of a curve table,
//                          and two additive offsets behind the variance scales
//
// One workgroup per utterance with the scalar kernel's stride loop, as in prosody.hip: an utterance's result depends on that utterance
// alone, and a thread meets the same rows in every loop, so the offsets need no barrier of their own.
#include "common.h"
#include "../../include/toucan_prosody_curves.h"

namespace tts {

namespace {

// block_sum is prosody.hip's (and sequence_ops.hip's), token for token: the same sums in the same order.
__device__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// _scale_variance with the scale of row r = scale * curves[r][col], then the offset curves[r][col + 2].  The mean is the scalar kernel's
// (non-zero entries of the whole utterance) and both reductions always run: no barrier under a divergent branch.  A row whose
// effective scale is exactly 1 is not written by the scale step - (v - avg) * 1 + avg is not v in fp32 - and the expression is the
// scalar kernel's three statements, which the compiler contracts alike in all three files.
__device__ void scale_variance_curve(float* seq, int r0, int r1, float scale, const float* __restrict__ curves, int col, float* red) {
  float s = 0.f, cnt = 0.f;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float v = seq[r];
    if (v != 0.0f) { s += v; cnt += 1.f; }
  }
  s = block_sum(s, red);
  cnt = block_sum(cnt, red);
  const float avg = s / cnt;  // empty selection -> NaN, as torch's mean of an empty tensor
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float* c = curves + (size_t)r * TTS_PROSODY_CURVE_COLUMNS;
    const float es = scale * c[col];
    if (es != 1.0f) {
      float v = seq[r] - avg;
      v = v * es;
      v = v + avg;
      seq[r] = v < 0.0f ? 0.0f : v;
    }
    const float o = c[col + 2];
    if (o != 0.0f) {
      float v = seq[r];
      if (v != 0.0f) {  // unvoiced rows stay unvoiced, non-phoneme rows keep energy 0
        v = v + o;
        seq[r] = v < 0.0f ? 0.0f : v;
      }
    }
  }
}

// scales == nullptr: every utterance's four scales are 1
__global__ __launch_bounds__(256) void prosody_control_c_kernel(const float* __restrict__ text, int ld_text, float* pitch, float* energy,
                                                                int* dur, const int* __restrict__ seq_begin,
                                                                const int* __restrict__ seq_end, const float* __restrict__ scales,
                                                                const float* __restrict__ curves) {
  __shared__ float red[4];
  const int u = blockIdx.x;
  const int r0 = seq_begin[u], r1 = seq_end[u];
  float duration_scale = 1.0f, pitch_scale = 1.0f, energy_scale = 1.0f, pause_scale = 1.0f;
  if (scales) {
    const float* s = scales + (size_t)u * 4;
    duration_scale = s[0]; pitch_scale = s[1]; energy_scale = s[2]; pause_scale = s[3];
  }
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float* f = text + (size_t)r * ld_text;
    if (f[61] == 0.0f) pitch[r] = 0.0f;
    if (f[15] == 0.0f) energy[r] = 0.0f;
    int d = dur[r];
    if (f[21] == 1.0f) d = 0;
    if (f[16] == 1.0f && pause_scale != 1.0f) d = (int)rintf((float)d * pause_scale);
    const float ed = duration_scale * curves[(size_t)r * TTS_PROSODY_CURVE_COLUMNS];
    if (ed != 1.0f) d = (int)rintf((float)d * ed);
    dur[r] = d;
  }
  __syncthreads();
  scale_variance_curve(pitch, r0, r1, pitch_scale, curves, 1, red);
  scale_variance_curve(energy, r0, r1, energy_scale, curves, 2, red);
}

}  // namespace

int prosody_control_c(const float* text, int ld_text, float* pitch, float* energy, int* dur, const int* sb, const int* se, int n_seq,
                      const float* scales, const float* curves, hipStream_t st) {
  TTS_CHECK_ARG(n_seq >= 0, "prosody_control_c: n_seq %d is negative", n_seq);
  if (n_seq == 0) return TTS_OK;
  TTS_CHECK_ARG(text && pitch && energy && dur && sb && se && curves, "prosody_control_c: null pointer");
  TTS_CHECK_ARG(ld_text >= 62, "prosody_control_c: ld_text %d < 62 feature columns", ld_text);
  hipLaunchKernelGGL(prosody_control_c_kernel, dim3(n_seq), dim3(256), 0, st, text, ld_text, pitch, energy, dur, sb, se, scales, curves);
  return launch_status("prosody_control_c");
}

}  // namespace tts

extern "C" {
int tts_prosody_control_c(const float* text, int32_t ld_text, float* pitch, float* energy, int32_t* dur, const int32_t* seq_begin,
                          const int32_t* seq_end, int32_t n_seq, const float* scales, const float* curves, tts_stream_t stream) {
  return tts::prosody_control_c(text, ld_text, pitch, energy, dur, seq_begin, seq_end, n_seq, scales, curves, static_cast<hipStream_t>(stream));
}
}  // extern "C"
