// Sample-rate conversion of a ragged batch of waveforms: polyphase windowed-sinc interpolation by the rational factor new / orig
// with torchaudio.transforms.Resample's defaults (include/toucan_resample.h holds the formula, DESIGN.md section 13 the decisions),
// float32 or PCM16 out.
//
//   tts_resample               one launch per ragged batch; whole utterances or the continuation of streamed ones
//   tts_resample_tile_outputs  outputs per workgroup
//
// Output m = i new + p of an utterance is sum_j k[p][j] x[i orig + j - w].  A workgroup of 256 threads produces RS_TILE consecutive
// outputs of one utterance, four per thread, 256 apart, so that a wavefront's 64 outputs are neighbours: their stores coalesce,
// their coefficients k[.][j] are neighbours in the transposed table, and their samples are the same or nearly the same addresses.
// The samples come through the vector L1 (a workgroup's window is a few KB); the table is staged in LDS when it fits 64 KiB and
// read through L1 / L2 otherwise (every wavefront of a workgroup walks the rows j in step, so a row is fetched from L2 about once
// per workgroup).
//
// Batch and chunk independence: every output is ONE chain of K fused multiply-adds, j = 0 .. K - 1, starting from 0, on the table
// row of its phase and its K samples (0 where the buffer holds none).  Nothing in the chain depends on the thread, the workgroup,
// the utterance's place in the batch or where the buffer starts.
#include "common.h"
#include "../../include/toucan_resample.h"

namespace tts {

constexpr int RS_THREADS = 256;
constexpr int RS_PER_THREAD = 4;
constexpr int RS_TILE = RS_THREADS * RS_PER_THREAD;

template <bool PCM>
__device__ __forceinline__ void store_sample(void* y, int64_t at, float v) {
  if constexpr (PCM) {
    // float2pcm: scale, saturate, let the integer conversion drop the fraction
    const float s = fminf(fmaxf(v * 32768.0f, -32768.0f), 32767.0f);
    static_cast<int16_t*>(y)[at] = (int16_t)(int)s;
  } else {
    static_cast<float*>(y)[at] = v;
  }
}

template <bool TAB_LDS, bool PCM>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                              const TtsResampleSpan* __restrict__ spans, void* __restrict__ y, int orig,
                                                              int nw, int w, int K) {
  extern __shared__ float lds_table[];
  const TtsResampleSpan s = spans[blockIdx.y];
  const int tid = threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * RS_TILE;
  if (o0 >= s.out_count) return;  // the whole workgroup: before any barrier
  const float* tab = table;
  if constexpr (TAB_LDS) {
    for (int e = tid; e < nw * K; e += RS_THREADS) lds_table[e] = table[e];
    __syncthreads();
    tab = lds_table;
  }
  // Buffer index of the chain's sample j = 0: of the tile's first output (the smallest) and of its last (the largest).
  const int64_t m_first = s.out_first + o0, m_last = m_first + RS_TILE - 1;
  const int64_t base_first = m_first / nw * orig - w - s.pos0, base_last = m_last / nw * orig - w - s.pos0;
  int off[RS_PER_THREAD], p[RS_PER_THREAD];
  int64_t base[RS_PER_THREAD];
  float acc[RS_PER_THREAD];
#pragma unroll
  for (int r = 0; r < RS_PER_THREAD; ++r) {
    const int64_t m = m_first + tid + r * RS_THREADS;
    const int64_t i = m / nw;
    p[r] = (int)(m - i * nw);
    if (p[r] < 0) p[r] += nw;  // (a negative out_first is the caller's mistake; the table is still read inside its rows)
    base[r] = i * orig - w - s.pos0;
    off[r] = (int)(base[r] - base_first);  // at most (RS_TILE / new + 1) orig
    acc[r] = 0.0f;
  }
  if (o0 + RS_TILE <= s.out_count && base_first >= 0 && base_last + K <= s.n_held) {
    // the whole tile is asked for and the buffer holds every sample it reads: the chain without the zero fill (the same chain)
    const float* xt = x + s.in_begin + base_first;
#pragma unroll 4
    for (int j = 0; j < K; ++j) {
      const float* row = tab + j * nw;
#pragma unroll
      for (int r = 0; r < RS_PER_THREAD; ++r) acc[r] = __builtin_fmaf(row[p[r]], xt[off[r] + j], acc[r]);
    }
  } else {
    const float* xb[RS_PER_THREAD];
    int lo[RS_PER_THREAD], hi[RS_PER_THREAD];
#pragma unroll
    for (int r = 0; r < RS_PER_THREAD; ++r) {
      // the taps j in [lo, hi) are the ones the buffer holds; an output past out_count gets none and is not stored
      const int64_t first = -base[r], past = s.n_held - base[r];
      lo[r] = (int)(first < 0 ? 0 : (first > K ? K : first));
      hi[r] = o0 + tid + r * RS_THREADS < s.out_count ? (int)(past < 0 ? 0 : (past > K ? K : past)) : 0;
      xb[r] = x + s.in_begin + base[r];  // dereferenced at [lo, hi) only
    }
    for (int j = 0; j < K; ++j) {
      const float* row = tab + j * nw;
#pragma unroll
      for (int r = 0; r < RS_PER_THREAD; ++r) {
        const float v = (j >= lo[r] && j < hi[r]) ? xb[r][j] : 0.0f;
        acc[r] = __builtin_fmaf(row[p[r]], v, acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RS_PER_THREAD; ++r) {
    const int64_t o = o0 + tid + r * RS_THREADS;
    if (o < s.out_count) store_sample<PCM>(y, s.out_begin + o, acc[r]);
  }
}

static int gcd_int(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

int resample(const float* x, const float* table, const TtsResampleSpan* spans, int batch, int64_t max_out_count, int orig, int nw, int w,
             int pcm16, void* y, hipStream_t st) {
  TTS_CHECK_ARG(orig >= 1 && nw >= 1 && orig <= TTS_RESAMPLE_MAX_FACTOR && nw <= TTS_RESAMPLE_MAX_FACTOR,
                "resample: the reduced ratio %d / %d is outside 1 .. TTS_RESAMPLE_MAX_FACTOR = %d", nw, orig, TTS_RESAMPLE_MAX_FACTOR);
  TTS_CHECK_ARG(gcd_int(orig, nw) == 1, "resample: orig %d and new %d are not coprime", orig, nw);
  TTS_CHECK_ARG(w >= 0 && w <= 8 * TTS_RESAMPLE_MAX_FACTOR, "resample: w %d is outside 0 .. %d", w, 8 * TTS_RESAMPLE_MAX_FACTOR);
  TTS_CHECK_ARG(pcm16 == 0 || pcm16 == 1, "resample: pcm16 is 0 or 1");
  TTS_CHECK_ARG(batch >= 0 && batch <= 65535 && max_out_count >= 0, "resample: batch %d is outside 0 .. 65535 or max_out_count negative", batch);
  const int64_t tiles = (max_out_count + RS_TILE - 1) / RS_TILE;
  TTS_CHECK_ARG(tiles <= 0x7fffffff, "resample: max_out_count needs more than 2^31 - 1 workgroups per utterance");
  if (batch == 0 || tiles == 0) return TTS_OK;
  TTS_CHECK_ARG(x && table && spans && y, "resample: null pointer");
  const int K = 2 * w + orig;
  const size_t table_bytes = (size_t)K * nw * sizeof(float);  // at most (16 K + 1 K) * 1 K * 4 B: far inside int
  const dim3 grid((unsigned)tiles, (unsigned)batch), block(RS_THREADS);
  if (table_bytes <= TTS_RESAMPLE_LDS_TABLE_BYTES) {
    if (pcm16) hipLaunchKernelGGL((resample_kernel<true, true>), grid, block, table_bytes, st, x, table, spans, y, orig, nw, w, K);
    else hipLaunchKernelGGL((resample_kernel<true, false>), grid, block, table_bytes, st, x, table, spans, y, orig, nw, w, K);
  } else {
    if (pcm16) hipLaunchKernelGGL((resample_kernel<false, true>), grid, block, 0, st, x, table, spans, y, orig, nw, w, K);
    else hipLaunchKernelGGL((resample_kernel<false, false>), grid, block, 0, st, x, table, spans, y, orig, nw, w, K);
  }
  return launch_status("resample");
}

}  // namespace tts

extern "C" {
int tts_resample_tile_outputs(void) { return tts::RS_TILE; }
int tts_resample(const float* x, const float* table, const TtsResampleSpan* spans, int32_t batch, int64_t max_out_count, int32_t orig,
                 int32_t new_, int32_t w, int32_t pcm16, void* y, tts_stream_t stream) {
  return tts::resample(x, table, spans, batch, max_out_count, orig, new_, w, pcm16, y, static_cast<hipStream_t>(stream));
}
}  // extern "C"
