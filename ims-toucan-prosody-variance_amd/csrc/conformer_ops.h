// Row arithmetic that a stand-alone kernel and the fused Conformer kernels (conformer_conv.hip) both evaluate: one instance each,
// so that every kernel rounds (and contracts) it alike and a fused launch gives the bits of the launches it replaces.
#pragma once
#include "common.h"

namespace tts {

constexpr int LN_MAX_PER_LANE = 8;  // channels <= 512

// wave_sum of NR independent values, step by step: the NR shuffles of a step are in flight together (a wavefront that reduces
// row after row waits out the cross-lane latency twelve times per row); per value it is wave_sum's arithmetic
template <int NR>
__device__ __forceinline__ void wave_sum_rows(float (&v)[NR]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    float t[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) t[r] = __shfl_xor(v[r], o, 64);
    if constexpr (NR > 1) __builtin_amdgcn_sched_barrier(0);  // (else the scheduler pairs every shuffle with its add again: one in flight)
#pragma unroll
    for (int r = 0; r < NR; ++r) v[r] += t[r];
    if constexpr (NR > 1) __builtin_amdgcn_sched_barrier(0);
  }
}

// Layers/LayerNorm.py:24-36 on NR rows by one wavefront: lane l holds channels l, l + 64, ... - vin[r][i], g[i], b[i] are row r, gamma
// and beta at channel l + 64 i (anything past c: v is taken as 0 there and o is 0).  Two-pass fp32 statistics (mean, then centred
// second moment) like ATen.  The rows are independent: NR only lets their reductions overlap.
template <int NR>
__device__ __forceinline__ void layernorm_rows(const float (&vin)[NR][LN_MAX_PER_LANE], int lane, int c, float eps, const float (&g)[LN_MAX_PER_LANE],
                                               const float (&b)[LN_MAX_PER_LANE], float (&o)[NR][LN_MAX_PER_LANE]) {
  float v[NR][LN_MAX_PER_LANE];
  float s[NR], q[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_PER_LANE; ++i) {
      const int ch = lane + 64 * i;
      v[r][i] = ch < c ? vin[r][i] : 0.f;
      s[r] += v[r][i];
    }
  }
  wave_sum_rows(s);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const float mean = s[r] / (float)c;
    s[r] = mean;
    q[r] = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAX_PER_LANE; ++i) {
      const int ch = lane + 64 * i;
      const float dlt = ch < c ? v[r][i] - mean : 0.f;
      q[r] += dlt * dlt;
    }
  }
  wave_sum_rows(q);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const float mean = s[r];
    const float var = q[r] / (float)c;
    const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
    for (int i = 0; i < LN_MAX_PER_LANE; ++i) {
      const int ch = lane + 64 * i;
      o[r][i] = ch < c ? (v[r][i] - mean) * rstd * g[i] + b[i] : 0.f;
    }
  }
}

// Depthwise conv (K taps, BatchNorm folded) + Swish of one output: the taps in ascending order on win[i] .. win[i + K - 1]
// (Layers/Convolution.py:50-51, Swish.py:18)
template <int K, int N>
__device__ __forceinline__ float dwconv_swish_value(const float (&wk)[K], const float (&win)[N], int i, float bias) {
  float a = bias;
#pragma unroll
  for (int j = 0; j < K; ++j) a = fmaf(wk[j], win[i + j], a);
  return a * (1.0f / (1.0f + expf(-a)));
}

}  // namespace tts
