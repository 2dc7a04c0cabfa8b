// The PostFlow in the forward direction (Glow.py:342-391 with infer=False): the per-row part of a flow step and the reduction of the
// latent to the glow loss (include/toucan_score.h).  The convs of the coupling blocks are tts_conv1d launches sequenced by
// tts_postflow_nll (pipeline.hip); nothing here is on the synthesis path.
//
// A squeezed row is 160 floats ([frame 2r | frame 2r + 1]) and every kernel here reads and writes it once: they are HBM-stream
// kernels.  Lane k of a row's 20 lanes owns the channels 4k .. 4k+3 of both halves - two 16-byte loads - which are exactly the two
// InvConvNear groups 2k and 2k+1 (group g mixes the channels 2g, 2g+1, 80+2g, 80+2g+1: Glow.py:102-103), so the 4x4 mix stays in
// registers.  A wavefront carries three rows (60 of its 64 lanes), a workgroup twelve.
//
// The arithmetic of a row is fp64 from the fp32 inputs to ONE rounding of each output (exp, the affine steps and the 4-term mix):
// the products of two floats are exact in fp64, so an output is the float nearest to the float64 result whatever cancels in it.
// At two 16-byte loads per four exps the fp64 work stays under the stream time.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "../../include/toucan_score.h"

namespace tts {

namespace {

constexpr int GF_C = 160, GF_HALF = 80, GF_ROW_LANES = 20, GF_WAVE_ROWS = 3, GF_THREADS = 256;
constexpr int GF_BLOCK_ROWS = TTS_GLOW_FORWARD_BLOCK_ROWS;
constexpr int GF_MAX_BLOCKS = TTS_GLOW_FORWARD_GRID_ROWS / GF_BLOCK_ROWS;  // more rows: the grid strides
static_assert(GF_BLOCK_ROWS == GF_WAVE_ROWS * (GF_THREADS / 64) && GF_MAX_BLOCKS * GF_BLOCK_ROWS == TTS_GLOW_FORWARD_GRID_ROWS, "toucan_score.h");

template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* p) {
  if constexpr (VEC) return *reinterpret_cast<const float4*>(p);
  else return make_float4(p[0], p[1], p[2], p[3]);
}
template <bool VEC>
__device__ __forceinline__ void st4(float* p, float4 v) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
}

// z[o] = sum_n W[o][n] v[n] over one group's slots (slot n = 2 a + r of channel a * 80 + 2 g + r), fp64
__device__ __forceinline__ void mix4(const double* __restrict__ W, double& v0, double& v1, double& v2, double& v3) {
  double z[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) z[o] = fma(W[o * 4 + 3], v3, fma(W[o * 4 + 2], v2, fma(W[o * 4 + 1], v1, W[o * 4 + 0] * v0)));
  v0 = z[0]; v1 = z[1]; v2 = z[2]; v3 = z[3];
}

// First half (ml): the coupling of block b, x1 = m + exp(logs) x1, and row_logdet[r] += sum_80 logs.
// Second half (w): ActNorm and InvConvNear of block b + 1, x = W (bias + exp(an_logs) x) group by group.
// Both: the coupling's output goes on in fp64, rounded once after the mix.
template <bool VEC>
__global__ __launch_bounds__(GF_THREADS) void glow_forward_rows_kernel(float* __restrict__ x, int ldx, int rows, const float* __restrict__ ml,
                                                                       int ld_ml, double* __restrict__ row_logdet, const float* __restrict__ w,
                                                                       const float* __restrict__ an_bias, const float* __restrict__ an_logs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / GF_ROW_LANES, k = lane - sub * GF_ROW_LANES;  // sub 3: the four lanes without a row
  const int base = sub * GF_ROW_LANES, c0 = 4 * k;
  double W[16], sc[8], bi[8];
  if (w) {  // this lane's channels are the same in every row
#pragma unroll
    for (int i = 0; i < 16; ++i) W[i] = (double)w[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sc[i] = exp((double)an_logs[c0 + i]);
      bi[i] = (double)an_bias[c0 + i];
      sc[4 + i] = exp((double)an_logs[GF_HALF + c0 + i]);
      bi[4 + i] = (double)an_bias[GF_HALF + c0 + i];
    }
  }
  for (long long r0 = ((long long)blockIdx.x * (GF_THREADS / 64) + wave) * GF_WAVE_ROWS; r0 < rows; r0 += (long long)gridDim.x * GF_BLOCK_ROWS) {
    const long long r = r0 + sub;
    const bool live = sub < GF_WAVE_ROWS && r < rows;
    float* xr = x + (size_t)(live ? r : 0) * ldx;
    double A[4] = {0, 0, 0, 0}, B[4] = {0, 0, 0, 0};
    if (live) {
      if (w) {
        const float4 a = ld4<VEC>(xr + c0);
        A[0] = a.x; A[1] = a.y; A[2] = a.z; A[3] = a.w;
      }
      const float4 b = ld4<VEC>(xr + GF_HALF + c0);
      B[0] = b.x; B[1] = b.y; B[2] = b.z; B[3] = b.w;
    }
    if (ml) {
      double s = 0.0;
      if (live) {
        const float* mr = ml + (size_t)r * ld_ml;
        const float4 m = ld4<VEC>(mr + c0), lg = ld4<VEC>(mr + GF_HALF + c0);
        B[0] = fma(exp((double)lg.x), B[0], (double)m.x);
        B[1] = fma(exp((double)lg.y), B[1], (double)m.y);
        B[2] = fma(exp((double)lg.z), B[2], (double)m.z);
        B[3] = fma(exp((double)lg.w), B[3], (double)m.w);
        s = ((double)lg.x + (double)lg.y) + ((double)lg.z + (double)lg.w);
      }
      // the row's 20 partial sums: lanes 16 .. 19 onto 0 .. 3, then a butterfly over 0 .. 15 - one order for every row.  Every lane
      // shuffles (lanes 16 .. 19 and a wave's last four read partners they do not use)
      double t = __shfl(s, (base + k + 16) & 63, 64);
      if (k < 4) s += t;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        t = __shfl(s, (base + (k ^ o)) & 63, 64);
        s += t;
      }
      if (live && k == 0) row_logdet[r] += s;  // (one writer per row)
    }
    if (!live) continue;
    if (w) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        A[i] = fma(sc[i], A[i], bi[i]);
        B[i] = fma(sc[4 + i], B[i], bi[4 + i]);
      }
      mix4(W, A[0], A[1], B[0], B[1]);
      mix4(W, A[2], A[3], B[2], B[3]);
      st4<VEC>(xr + c0, make_float4((float)A[0], (float)A[1], (float)A[2], (float)A[3]));
    }
    st4<VEC>(xr + GF_HALF + c0, make_float4((float)B[0], (float)B[1], (float)B[2], (float)B[3]));
  }
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int glow_forward_rows(float* x, int ldx, int rows, const float* ml, int ld_ml, double* row_logdet, const float* w, const float* an_bias,
                      const float* an_logs, hipStream_t st) {
  TTS_CHECK_ARG(x && ldx >= GF_C && rows >= 0, "glow_forward_rows: null x / row stride %d < 160 / %d rows", ldx, rows);
  TTS_CHECK_ARG(ml || w, "glow_forward_rows: neither half was given");
  TTS_CHECK_ARG(!ml || (row_logdet && ld_ml >= GF_C), "glow_forward_rows: the coupling half needs row_logdet and a row stride >= 160 (%d)", ld_ml);
  TTS_CHECK_ARG(!w || (an_bias && an_logs), "glow_forward_rows: the ActNorm / InvConv half needs w, an_bias and an_logs");
  if (rows == 0) return TTS_OK;
  const int blocks = (int)std::min<long long>(((long long)rows + GF_BLOCK_ROWS - 1) / GF_BLOCK_ROWS, GF_MAX_BLOCKS);
  const bool vec = al16(x) && (ldx & 3) == 0 && (!ml || (al16(ml) && (ld_ml & 3) == 0));
  if (vec)
    hipLaunchKernelGGL(glow_forward_rows_kernel<true>, dim3(blocks), dim3(GF_THREADS), 0, st, x, ldx, rows, ml, ld_ml, row_logdet, w, an_bias, an_logs);
  else
    hipLaunchKernelGGL(glow_forward_rows_kernel<false>, dim3(blocks), dim3(GF_THREADS), 0, st, x, ldx, rows, ml, ld_ml, row_logdet, w, an_bias, an_logs);
  return launch_status("glow_forward_rows");
}

// ---- the glow loss of each utterance from its latent rows, one workgroup per utterance -----------------------------------------
// Wave v takes the utterance's rows v, v + 4, ...: 40 lanes square a row's 160 values in fp64, wave_sum (wave_ops.h) adds them, lane 0 adds the
// row's two parts to the wave's sums; thread 0 adds the four waves' sums in order.  Nothing depends on the batch.
constexpr double HALF_LOG_2PI = 0.91893853320467274178;

template <bool VEC>
__global__ __launch_bounds__(GF_THREADS) void glow_nll_reduce_kernel(const float* __restrict__ z, int ldz, const double* __restrict__ row_logdet,
                                                                     const int* __restrict__ row_begin, const int* __restrict__ n_rows,
                                                                     const int* __restrict__ n_frames, double logdet_per_row,
                                                                     float* __restrict__ loss, float* __restrict__ row_parts) {
  __shared__ double part[GF_THREADS / 64][2];
  const int u = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = row_begin[u], n = n_rows[u];
  double prior = 0.0, logdet = 0.0;
  for (int i = wave; i < n; i += GF_THREADS / 64) {
    const size_t r = (size_t)r0 + i;
    double q = 0.0;
    if (lane < GF_C / 4) {
      const float4 v = ld4<VEC>(z + r * ldz + 4 * lane);
      q = ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
    q = wave_sum(q);
    q = 0.5 * q + GF_C * HALF_LOG_2PI;
    const double l = row_logdet[r];
    if (lane == 0 && row_parts) {
      row_parts[2 * r] = (float)q;
      row_parts[2 * r + 1] = (float)(l + logdet_per_row);
    }
    prior += q;
    logdet += l;
  }
  if (lane == 0) {
    part[wave][0] = prior;
    part[wave][1] = logdet;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double p = 0.0, l = 0.0;
    for (int v = 0; v < GF_THREADS / 64; ++v) {
      p += part[v][0];
      l += part[v][1];
    }
    l += (double)n * logdet_per_row;
    // Glow.py:354-356: the prior's mean runs over the squeezed rows, the log-determinant is divided by the unsqueezed length
    loss[u] = n > 0 ? (float)(p / ((double)GF_C * n) - l / ((double)GF_HALF * n_frames[u])) : __builtin_nanf("");
  }
}

int glow_nll_reduce(const float* z, int ldz, const double* row_logdet, const int* row_begin, const int* n_rows, const int* n_frames, int batch,
                    double logdet_per_row, float* loss, float* row_parts, hipStream_t st) {
  TTS_CHECK_ARG(z && row_logdet && row_begin && n_rows && n_frames && loss, "glow_nll_reduce: null pointer");
  TTS_CHECK_ARG(ldz >= GF_C && batch >= 0, "glow_nll_reduce: row stride %d < 160 / batch %d", ldz, batch);
  if (batch == 0) return TTS_OK;
  if (al16(z) && (ldz & 3) == 0)
    hipLaunchKernelGGL(glow_nll_reduce_kernel<true>, dim3(batch), dim3(GF_THREADS), 0, st, z, ldz, row_logdet, row_begin, n_rows, n_frames,
                       logdet_per_row, loss, row_parts);
  else
    hipLaunchKernelGGL(glow_nll_reduce_kernel<false>, dim3(batch), dim3(GF_THREADS), 0, st, z, ldz, row_logdet, row_begin, n_rows, n_frames,
                       logdet_per_row, loss, row_parts);
  return launch_status("glow_nll_reduce");
}

}  // namespace

}  // namespace tts

extern "C" {
int tts_glow_forward_rows(float* x, int32_t ldx, int32_t rows, const float* ml, int32_t ld_ml, double* row_logdet, const float* w,
                          const float* an_bias, const float* an_logs, tts_stream_t stream) {
  return tts::glow_forward_rows(x, ldx, rows, ml, ld_ml, row_logdet, w, an_bias, an_logs, reinterpret_cast<hipStream_t>(stream));
}
int tts_glow_nll_reduce(const float* z, int32_t ldz, const double* row_logdet, const int32_t* row_begin, const int32_t* n_rows,
                        const int32_t* n_frames, int32_t batch, double logdet_per_row, float* loss, float* row_parts, tts_stream_t stream) {
  return tts::glow_nll_reduce(z, ldz, row_logdet, row_begin, n_rows, n_frames, batch, logdet_per_row, loss, row_parts,
                              reinterpret_cast<hipStream_t>(stream));
}
}
