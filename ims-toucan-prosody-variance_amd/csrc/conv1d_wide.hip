// The wide tile of tts_conv1d: 256 rows x 256 columns per workgroup for plain 16-bit convs (bf16 / fp16 tensors in and out,
// LINEAR mode, no prologue), both operands carried into LDS by global_load_lds_dwordx4 (LDS-DMA: no staging registers, no ds_write
// pass).  Eight wavefronts, 2 (rows) x 4 (columns); each owns 128 x 64 outputs as 4 x 2 accumulators of
// v_mfma_f32_32x32x16_{bf16,f16}, about one workgroup per CU.  Per k-step a wavefront issues 6 ds_read_b128 for 8 matrix
// instructions (the 128 x 128 tile of conv1d.hip: 4 for 4).
//
// Arithmetic: the same matrix instruction and, per output element, the same accumulation order as conv1d_kernel (64-channel slab
// outer, tap inner, k ascending in 16-channel steps, weights as the A operand) and the same epilogue (conv_epilogue_t, bias from
// LDS), so the result is bit-identical to the 128 x 128 and the 64-row forms; tests/test_gpu_conv_wide_tile.py asserts it.
//
// LDS (one array):  [2] activation windows | [2] weight slabs | bias.
//   window: (256 + (taps-1) dil, rounded up to 8) rows x 64 channels of the 16-bit input = 128-byte rows, LINEAR (a DMA instruction
//     writes wave base + lane x 16 bytes: 8 whole rows), the 16-byte unit of channel group g of window row r stored at position
//     g ^ ((r >> 1) & 7) of its row - the permutation is applied to the per-lane SOURCE address and again by the reader.  Any 16
//     consecutive rows of one channel group then cover all sixteen 16-byte slots of the 256-byte bank row: the A-fragment
//     ds_read_b128 (32 consecutive rows per half wave, at any tap offset) is conflict-free.
//   weight slab: the packed layout [cin/8][wn][8] gives, per 8-channel group, 256 columns x 16 bytes = 4 KB contiguous in global
//     memory; the slab is the 8 groups of a 64-channel slab of one tap, [8][256][8] elements = 32 KB, 32 DMA instructions of 1 KB.
//   The window of slab ch+1 is requested at the first step of slab ch, the weights of step s+1 at step s.
//
// Synchronisation (two buffers each): per step (slab, tap)  s_waitcnt vmcnt(0) - barrier - request the next operands - multiply.
// A wavefront waits for its OWN requests, then the barrier publishes everybody's: the readers read only behind that barrier (an
// LDS-DMA is ordered for a ds_read by nothing but the issuing wavefront's vmcnt plus a barrier the reader has passed).  The request
// overwrites the buffer read one step (weights) / one slab (window) ago, which every wavefront has left when it passed the barrier.
//
// Zero padding at the utterance's edges: the DMA source rows are CLAMPED into the utterance (always a valid address) and the
// window rows outside [seq_begin, seq_end) are zeroed in LDS afterwards, by the wavefront that requested them: each lane overwrites
// exactly the 16 bytes its own DMA instruction wrote, behind its own s_waitcnt vmcnt(0) (so the DMA has landed and cannot overwrite
// the zeros) and in front of the barrier that publishes the window.  The branch is workgroup-uniform and taken by edge tiles only.
// (A buffer descriptor with out-of-range reads returning zero would need one descriptor per tile and negative row offsets.)
//
// TTS_IO_POLYPHASE (the polyphase up-samplers, taps == 3): tap 0 multiplies only zeros for the columns >= wn / 2, tap 2 for the
// columns < wn / 2.  A workgroup whose 256 columns lie wholly in such a half skips the step (no DMA, no barrier); otherwise a
// wavefront whose 64 columns do skips its matrix instructions.  Finite sums are unchanged (only the sign of an exact zero can differ).
#include "common.h"
#include "conv_epilogue.h"

namespace tts {

namespace {

constexpr int WIDE_BM = 256, WIDE_BN = 256, WIDE_BK = 64, WIDE_THREADS = 512;
constexpr int WIDE_ROW_BYTES = WIDE_BK * 2;                // a window row: 64 channels, 16-bit
constexpr int WIDE_SLAB_BYTES = WIDE_BK * WIDE_BN * 2;     // a weight slab: 32 KB

__host__ __device__ inline int wide_win_rows(int taps, int dil) { return (WIDE_BM + (taps - 1) * dil + 7) & ~7; }
inline size_t wide_lds_bytes(int taps, int dil) {
  return (size_t)2 * wide_win_rows(taps, dil) * WIDE_ROW_BYTES + 2 * WIDE_SLAB_BYTES + 2 * WIDE_BN * sizeof(float);
}

__device__ __forceinline__ void wide_dma16(const void* src, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)lds_wave_base, 16, 0, 0);
}

template <bool F16>
__global__ __launch_bounds__(WIDE_THREADS) void conv1d_wide_kernel(const TtsConvDesc d) {
  constexpr int TM = 4, TN = 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];

  const TtsTile tile = d.tiles[blockIdx.x];
  const int n0 = blockIdx.y * WIDE_BN;
  const int win_rows = wide_win_rows(d.taps, d.dil);
  const int win_bytes = win_rows * WIDE_ROW_BYTES;
  unsigned char* const xs0 = lds_raw;                                      // [2][win_rows][128 B]
  unsigned char* const ws0 = lds_raw + 2 * win_bytes;                      // [2][8][256][16 B]
  float* const eb = reinterpret_cast<float*>(ws0 + 2 * WIDE_SLAB_BYTES);   // [2][256]: bias, per-utterance vector (none here: zeros)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int lrow = lane & 31, lk = lane >> 5;

  f32x16 acc[1][TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][i][j][r] = 0.0f;

  if (tid < WIDE_BN) {
    const int n = n0 + tid;
    eb[tid] = (d.bias && n < d.cout) ? d.bias[n] : 0.0f;
    eb[WIDE_BN + tid] = 0.0f;
  }

  // the taps this workgroup multiplies, and the ones this wavefront leaves out among them (TTS_IO_POLYPHASE)
  const bool poly = d.io_flags & TTS_IO_POLYPHASE;
  const int half = d.wn >> 1;
  const int tap_lo = (poly && n0 >= half) ? 1 : 0;
  const int tap_hi = (poly && n0 + WIDE_BN <= half) ? 2 : d.taps;
  const int wc0 = n0 + wn * 64;  // first column of this wavefront
  const int skip_tap = !poly ? -1 : (wc0 >= half ? 0 : (wc0 + 64 <= half ? 2 : -1));

  const int row_first = tile.row0 - d.pad_left;  // packed row of window row 0
  const bool edge = row_first < tile.seq_begin || row_first + win_rows > tile.seq_end;
  const unsigned short* __restrict__ xh = reinterpret_cast<const unsigned short*>(d.x);
  const unsigned short* __restrict__ W = reinterpret_cast<const unsigned short*>(d.w);
  const int n_chunks = d.cin / WIDE_BK;
  const int n_win_inst = win_rows >> 3;  // DMA instructions of a window: 8 rows each

  // window of channel slab ch -> buffer ch & 1: wavefront w issues the instructions w, w + 8, ...
  auto request_window = [&](int ch) __attribute__((always_inline)) {
    unsigned char* xb = xs0 + (ch & 1) * win_bytes;
    for (int i = wave; i < n_win_inst; i += 8) {
      const int wr = i * 8 + (lane >> 3);
      const int g = (lane & 7) ^ ((wr >> 1) & 7);  // channel group stored at this lane's position of the row
      const int gr = row_first + wr;
      const int grc = gr < tile.seq_begin ? tile.seq_begin : (gr >= tile.seq_end ? tile.seq_end - 1 : gr);
      wide_dma16(xh + (size_t)grc * d.ldx + ch * WIDE_BK + g * 8, xb + i * 1024);
    }
  };
  // ... and the same lanes zero what they fetched for rows outside the utterance (behind their own vmcnt(0), see the head comment)
  auto zero_window_edges = [&](int ch) __attribute__((always_inline)) {
    unsigned char* xb = xs0 + (ch & 1) * win_bytes;
    for (int i = wave; i < n_win_inst; i += 8) {
      const int gr = row_first + i * 8 + (lane >> 3);
      if (gr < tile.seq_begin || gr >= tile.seq_end) *reinterpret_cast<uint4*>(xb + i * 1024 + lane * 16) = make_uint4(0, 0, 0, 0);
    }
  };
  // weight slab of (slab ch, tap) -> buffer buf: 32 instructions of 1 KB, four per wavefront
  auto request_weights = [&](int ch, int tap, int buf) __attribute__((always_inline)) {
    unsigned char* wb = ws0 + buf * WIDE_SLAB_BYTES;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = q * 8 + wave;  // (8-channel group, 64-column part)
      const int kb = idx >> 2, part = idx & 3;
      const size_t goff = (((size_t)tap * (d.cin_pad >> 3) + ch * 8 + kb) * d.wn + n0 + part * 64 + lane) * 8;
      wide_dma16(W + goff, wb + idx * 1024);
    }
  };

  request_window(0);
  request_weights(0, tap_lo, 0);
  bool zero_pending = edge;  // a requested window whose edge rows are not zeroed yet (the window of slab `zero_ch`)
  int zero_ch = 0;

  int step = 0;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const unsigned char* xb = xs0 + (ch & 1) * win_bytes;
    for (int tap = tap_lo; tap < tap_hi; ++tap, ++step) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's requests have landed
      if (zero_pending) {
        zero_window_edges(zero_ch);
        zero_pending = false;
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // ... everybody's: window and slab of this step are visible
      {
        const bool last_tap = tap + 1 == tap_hi;
        const int nch = last_tap ? ch + 1 : ch, ntap = last_tap ? tap_lo : tap + 1;
        if (nch < n_chunks) request_weights(nch, ntap, (step + 1) & 1);
      }
      if (tap == tap_lo && ch + 1 < n_chunks) {
        request_window(ch + 1);
        zero_pending = edge;
        zero_ch = ch + 1;
      }
      if (tap == skip_tap) continue;  // (wave-uniform) this wavefront's columns of the tap are structural zeros
      const unsigned char* wb = ws0 + (step & 1) * WIDE_SLAB_BYTES;
      const int r0 = wm * 128 + lrow + tap * d.dil;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int g = ks * 2 + lk;
        bf16x8 a[TM], b[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const bf16x8*>(wb + (size_t)(g * WIDE_BN + wn * 64 + j * 32 + lrow) * 16);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int r = r0 + i * 32;
          a[i] = *reinterpret_cast<const bf16x8*>(xb + r * WIDE_ROW_BYTES + ((g ^ ((r >> 1) & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[0][i][j] = mfma16<F16>(b[j], a[i], acc[0][i][j]);  // transposed: weights = A operand (conv_epilogue_t)
      }
    }
  }
  // (eb was written before the first barrier; no DMA is in flight: the last step requested nothing)
  conv_epilogue_t<TM, TN, 1, false, true>(d, tile, n0, wm, wn, lrow, lk, acc, eb, WIDE_BN);
}

}  // namespace

// Is the call one the wide tile can run?  (the hosts ask before they build a 256-row table; conv1d_dispatch asks again and refuses)
const char* conv1d_wide_reject(const TtsConvDesc& d) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (d.compute != TTS_COMPUTE_BF16 && d.compute != TTS_COMPUTE_F16) return "compute must be bf16 or fp16";
  if (d.mode != TTS_MODE_LINEAR) return "mode must be LINEAR";
  if (!(d.io_flags & TTS_IO_X_BF16) || !(d.io_flags & TTS_IO_Y_BF16) || (d.res && !(d.io_flags & TTS_IO_RES_BF16))) return "x, y and res must be 16-bit tensors";
  if (((d.io_flags & TTS_IO_F16) != 0) != (d.compute == TTS_COMPUTE_F16)) return "the 16-bit tensors must be in the call's own format";
  if (d.pre_act != TTS_PRE_NONE) return "no pre-activation";
  if (d.seqvec || d.preadd || d.aux) return "no seqvec, preadd or aux";
  if (d.cin != d.cin_pad || d.cin % WIDE_BK != 0) return "cin must be unpadded and a multiple of 64";
  if (d.wn % WIDE_BN != 0 || d.cout > d.wn) return "wn must be a multiple of 256";
  if ((d.cout & 3) || (d.bias && !al16(d.bias))) return "cout must be a multiple of 4 and the bias 16-byte aligned";  // (conv_epilogue_t's vector path)
  if ((d.ldx & 7) || (d.ldy & 7) || (d.res && (d.ld_res & 7)) || !al16(d.x) || !al16(d.y) || !al16(d.w) || (d.res && !al16(d.res))) return "rows and pointers must be 16-byte aligned";
  if ((d.io_flags & TTS_IO_POLYPHASE) && d.taps != 3) return "TTS_IO_POLYPHASE needs taps == 3";
  if (wide_lds_bytes(d.taps, d.dil) > 160 * 1024) return "the window does not fit in 160 KiB of LDS";
  return nullptr;
}

int conv1d_wide_launch(const TtsConvDesc& d, hipStream_t st) {
  const char* why = conv1d_wide_reject(d);
  TTS_CHECK_ARG(why == nullptr, "conv1d: a 256-row tile table asks for the wide tile, which this call cannot take: %s", why);
  const size_t lds = wide_lds_bytes(d.taps, d.dil);
  dim3 grid(d.n_tiles, d.wn / WIDE_BN), block(WIDE_THREADS);
  auto launch = [&](auto k, unsigned long long& raised) {
    if (lds > 64 * 1024) {
      const hipError_t e = raise_lds_limit(reinterpret_cast<const void*>(k), raised);
      if (e != hipSuccess) {
        set_error("conv1d (wide): raising the dynamic LDS limit failed: %s", hipGetErrorString(e));
        return (int)TTS_E_LAUNCH;
      }
    }
    hipLaunchKernelGGL(k, grid, block, lds, st, d);
    return launch_status("conv1d (wide)");
  };
  static unsigned long long raised_bf16 = 0, raised_f16 = 0;  // devices on which the instantiation's limit is already raised
  if (d.compute == TTS_COMPUTE_F16) return launch(conv1d_wide_kernel<true>, raised_f16);
  return launch(conv1d_wide_kernel<false>, raised_bf16);
}

}  // namespace tts
