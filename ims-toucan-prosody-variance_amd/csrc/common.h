// Internal helpers shared by the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/toucan_tts.h"

namespace tts {

void set_error(const char* fmt, ...);

#define TTS_CHECK_ARG(cond, ...)   \
  do {                             \
    if (!(cond)) {                 \
      tts::set_error(__VA_ARGS__); \
      return TTS_E_ARG;            \
    }                              \
  } while (0)

inline int launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return TTS_E_LAUNCH;
  }
  return TTS_OK;
}

// Raise a kernel's dynamic-LDS limit to the CU's 160 KiB once per (instantiation, device): `mask` is the instantiation's
// static bit set of devices already done.  The first (eager) launch does it, so it never lands inside a stream capture.
// The runtime refuses a dynamic limit that does not fit beside the kernel's own __shared__ variables, so those are taken off the
// 160 KiB.  A failure is returned AND taken out of hipGetLastError, where the next launch_status would find it.
inline hipError_t raise_lds_limit(const void* kernel, unsigned long long& mask) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (mask & bit) return hipSuccess;
  int room = 160 * 1024;
  hipFuncAttributes attr;
  if (hipFuncGetAttributes(&attr, kernel) == hipSuccess) room -= (int)attr.sharedSizeBytes;
  else (void)hipGetLastError();
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, room);
  if (e == hipSuccess) mask |= bit;
  else (void)hipGetLastError();
  return e;
}

// tts_wavenet_layer with the block's conditioning conv (1 tap, 384 -> wc_n) computed inside the layer instead of read from
// d.cond (which is ignored): cond = g * wc[:, col0 .. col0 + 383] + bc[col0 .. col0 + 383], columns a | g, in the arithmetic of
// tts_conv1d's 16-bit path, so the layer's output is bit-identical to the two-launch form (wavenet.hip)
struct WavenetCond {
  const float* g;   // [rows, 384] fp32: the squeezed speaker / utterance conditioning, same packed rows as hs
  int ld_g;
  const void* wc;   // packed as for tts_conv1d(compute 1 / 2): [1][48][wc_n][8]
  int wc_n;         // 1536: four layers' columns
  int col0;         // this layer's first column (layer index * 384)
  const float* bc;  // bias [wc_n]
};
int wavenet_layer_cond(const TtsWavenetDesc& d, const WavenetCond& c, hipStream_t st);

// One coupling block of the PostFlow's reverse pass in one launch (wavenet.hip): h = start(x0), the four WaveNet layers, then on
// the block's skip sum - which never leaves the chip - [m | logs] = end(skip), the coupling x1 = (x1 - m) exp(-logs), the inverse
// 1x1 conv and ActNorm (glow_invconv_actnorm).  x in ([rows, 160] fp32, the packed rows of the squeezed layout), x_out likewise:
// a different buffer, because a workgroup reads the x0 halo rows that its neighbours rewrite and the inverse conv changes every
// channel.  The start conv as packed for tts_conv1d's 16-bit path ([1][cin_pad / 8][w0_n][8], only its first 192 columns are used),
// the layers' weights and the conditioning as for wavenet_layer_cond; layer i uses conditioning columns 384 i .. 384 i + 383;
// `end` as packed for tts_conv1d's fp32 path ([192][we_n], m in columns 0 .. 79, logs from column we_half), bias [m | logs].
// The tile table has wavenet_block_tile_rows() rows per tile.  pad_rows: the n_pad rows of x that lie in no tile (the squeezed
// row that holds the dropped last frame of an utterance with an odd frame count): they only pass the inverse conv and ActNorm, as
// they do in glow_invconv_actnorm, which runs over all rows.
struct WavenetBlock {
  const float* x; int ld_x;
  float* x_out; int ld_out;
  const void* w0; int w0_n; const float* b0;  // start: 80 -> 192
  const float* we; int we_n; int we_half; const float* be; float alpha;  // end: 192 -> 2 x 80, fp32; alpha: the conv's output scale
  const float *winv, *an_bias, *an_logs;      // inverse 1x1 conv [4][4], ActNorm [160]
  const int* pad_rows; int n_pad;
  const void* w1[4]; const float* b1[4];      // in_layer: packed [5][24][384][8], bias [384]
  const void* w2[4]; const float* b2[4];      // res_skip: packed [1][24][384][8] (last layer [1][24][192][8]), bias
  const float* g; int ld_g;
  const void* wc; int wc_n; const float* bc;
  const TtsTile* tiles; int n_tiles; int tile_rows;
  int compute;
};
int wavenet_block(const WavenetBlock& d, hipStream_t st);
int wavenet_block_tile_rows();

// The Conformer convolution module in one launch (conformer_conv.hip): y = x + pw2(swish(dwconv_bn(glu(pw1(LN(x)))))), width 192,
// depthwise kernel 31 (the decoder's), bit-identical to tts_layernorm + tts_conv1d (GLU) + tts_dwconv_swish + tts_conv1d (residual) on the
// 16-bit path.  y is a different buffer than x: a workgroup reads the halo rows that its neighbours own.  pw1 / pw2 as packed for
// tts_conv1d's 16-bit path ([1][24][w_n][8]; pw1's gate half starts at column w1_half, its bias is [value 192 | gate 192]).
// The tile table has conformer_conv_tile_rows(kernel) rows per tile.
struct ConformerConv {
  const float* x; int ld_x;
  float* y; int ld_y;
  const float *ln_g, *ln_b; float eps;
  const void* w1; int w1_n; int w1_half; const float* b1;
  const float *dw_w, *dw_b; int kernel;  // [kernel][192] (BatchNorm folded), [192]
  const void* w2; int w2_n; const float* b2;
  const TtsTile* tiles; int n_tiles; int tile_rows;
  int compute;
};
int conformer_conv(const ConformerConv& d, hipStream_t st);
int conformer_conv_tile_rows(int kernel);

// LayerNorm and a 1-tap 192 -> cout conv (cout a multiple of 96) in one launch (conformer_conv.hip): y = W LN(x) + bias, fp32 out,
// bit-identical to tts_layernorm + tts_conv1d on the 16-bit path.  w as packed for tts_conv1d ([1][24][w_n][8]); 128-row tile table.
struct LnLinear {
  const float* x; int ld_x;
  float* y; int ld_y;
  const float *ln_g, *ln_b; float eps;
  const void* w; int w_n; const float* bias; int cout;
  const TtsTile* tiles; int n_tiles; int tile_rows;
  int compute;
};
int ln_linear(const LnLinear& d, hipStream_t st);

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
  const __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: round to nearest even, NaN preserved
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf16_to_f32(unsigned short u) { return __builtin_bit_cast(float, (unsigned int)u << 16); }

// 16-bit element formats of the MFMA paths: bf16 (compute 1) or IEEE fp16 (compute 2, v_mfma_f32_32x32x16_f16).  Both convert
// round-to-nearest-even, two values per instruction (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32).  fp16 does not saturate: above 65504
// the conversion gives inf, below 2^-14 it rounds into subnormals (kept by the conversion, the LDS reads and the MFMAs: measured
// down to inputs of 2^-22, tests/test_gpu_dynamic_range.py).  The callers keep what leaves that window in a trained model (flow
// state, norm statistics, accumulators) in fp32; an fp16 operand or 16-bit HBM tensor is finite for inputs up to 2^13 times unit
// scale and spends the format's own budget down to 2^-14 ("The 16-bit kernels over the dynamic range").
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned short f32_to_f16(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
__device__ __forceinline__ float f16_to_f32(unsigned short u) { return (float)__builtin_bit_cast(_Float16, u); }
template <bool F16>
__device__ __forceinline__ unsigned short to16(float f) {
  if constexpr (F16) return f32_to_f16(f);
  else return f32_to_bf16(f);
}
template <bool F16>
__device__ __forceinline__ float from16(unsigned short u) {
  if constexpr (F16) return f16_to_f32(u);
  else return bf16_to_f32(u);
}
// (lo, hi) -> one dword of two 16-bit elements: one packed conversion either way (converted one by one and or-ed together, the
// bf16 pair cost two conversions, a shift and an or)
template <bool F16>
__device__ __forceinline__ unsigned int pack16(float lo, float hi) {
  const f32x2 v = {lo, hi};
  if constexpr (F16) return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, f16x2));
  else return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2));
}
// run-time format (tensors in HBM whose format is a flag of the call, TTS_IO_F16)
__device__ __forceinline__ float load16(unsigned short u, bool f16) { return f16 ? f16_to_f32(u) : bf16_to_f32(u); }
__device__ __forceinline__ unsigned short store16(float v, bool f16) { return f16 ? f32_to_f16(v) : f32_to_bf16(v); }

// v_mfma_f32_32x32x16_{bf16,f16}: same shape, same operand layout, same cycles
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// Operand streams written with inline-asm loads and hand-counted waits (conv1d.hip: the 1-tap rows form and the split-K form;
// wavenet.hip: the weight stream): the loads return in order, so before k-step s is consumed exactly (DEPTH-1) * L younger loads
// may stay in flight (L = loads per k-step).  Left to the compiler the same loop either had its 16-byte loads split into dwords
// (the fragments are consumed lane-element by lane-element) or drained every outstanding load at the loop head (it cannot count
// across the back edge); the asm is invisible to its counters, and each wait is followed by empty asm statements that
// "redefine" the registers just waited for (TTS_PIN), so no use can move above it.
#define TTS_GLOAD128(dst_, ptr_) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst_) : "v"(ptr_) : "memory")
#define TTS_GLOAD32(dst_, ptr_) asm volatile("global_load_dword %0, %1, off" : "=v"(dst_) : "v"(ptr_) : "memory")
#define TTS_WAIT_VM(n_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n_) : "memory")
#define TTS_PIN(r_) asm volatile("" : "+v"(r_))

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + __expf(-v)); }

// log correctly rounded to float32 (through double), independent of libm's float32 form
__device__ inline float log_rn(float x) { return (float)log((double)x); }

// Glow, reverse pass: the expressions that more than one kernel evaluates, in one place each so that every kernel contracts and
// rounds them alike (the coupling: tts_conv1d's epilogue and wavenet_block_kernel; the mix: glow_mix_kernel and wavenet_block_kernel).
//   coupling (Glow.py:301): x1 = (x1 - m) exp(-logs), m and logs with their biases already added
__device__ __forceinline__ float glow_coupling_value(float ax, float m, float logs) { return (ax - m) * expf(-logs); }
//   output slot o of a mixing group's inverse 1x1 conv, then ActNorm's inverse (Glow.py:124, :30-31); w = Winv, row-major [4][4];
//   an_scale = glow_actnorm_scale(logs) of the output channel (a kernel may keep it per channel instead of taking it per element)
__device__ __forceinline__ float glow_actnorm_scale(float an_logs) { return expf(-an_logs); }
__device__ __forceinline__ float glow_mix_value(const float (&w)[16], int o, float v0, float v1, float v2, float v3, float an_bias, float an_scale) {
  float z = w[o * 4 + 0] * v0;
  z = fmaf(w[o * 4 + 1], v1, z);
  z = fmaf(w[o * 4 + 2], v2, z);
  z = fmaf(w[o * 4 + 3], v3, z);
  return (z - an_bias) * an_scale;
}

}  // namespace tts

// the cross-lane reductions and scans (wave_sum, block_sum, wave_max, ...): kept reachable through this header for its users
#include "wave_ops.h"
