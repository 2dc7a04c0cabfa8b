// Two fused launches of the Conformer block (Layers/EncoderLayer.py:93-125), 16-bit MFMA configurations, model width 192:
//
//   conformer_conv_kernel   y = x + pw2( swish( dwconv_bn( glu( pw1( LN(x) ) ) ) ) )      (Layers/Convolution.py:31-55)
//   ln_linear_kernel        y = W LN(x) + b                                               (norm_mha + the q | k | v projection)
//
// Both give the bits of the launches they replace (tts_layernorm, tts_conv1d, tts_dwconv_swish): LayerNorm and the depthwise chain
// are the shared functions of conformer_ops.h, the products follow tts_conv1d's 16-bit forms (operands rounded to 16 bits, weights
// as the MFMA A operand, k ascending in steps of 16, one fp32 accumulator chain from zero) and the epilogues are epilogue_value.
//
// Common front half (256 threads = 4 wavefronts, 128 rows per workgroup, 32 per wavefront):
//   * a wavefront normalises its 32 rows exactly as layernorm_kernel does (lane = channel mod 64; 16 rows' reductions in flight together) and writes them as
//     16-bit elements into its part of an LDS window [128][192 + 8]; it then reads the window back transposed - lane = row, eight
//     consecutive channels per 16-channel k step - as the B operands xb[12], which stay in registers for the whole kernel;
//   * the weights stream through a two-stage LDS ring of 36 KB stages (36 fragments of 64 lanes x 16 B, each one ds_read_b128 per
//     lane) in the fragment order, taken straight from the [cin/8][cout][8] packing: stage s + 1 is requested into nine registers
//     per lane behind the barrier that opens stage s and written to the other stage at the end of stage s, so its latency hides
//     under the whole stage.  (Not global_load_lds: the compiler then waits for every outstanding LDS-DMA load - vmcnt(0) - in
//     front of the first LDS access it cannot tell from the ring, here the bias read right behind the first product, which put
//     the load latency back on every stage.)  Nothing else is loaded from global memory inside the loop (biases and depthwise
//     weights are copied to LDS up front), so the only wait of the loop is the one in front of the ring's writes.
//
// conformer_conv_kernel<K>: a workgroup stores TR = 128 - (K - 1) rows of one utterance (98 for the decoder's K = 31) and computes
// LN, pw1 and GLU on those plus H = (K - 1) / 2 halo rows a side; window rows outside the utterance are ZERO at the depthwise
// conv's input, as dwconv_swish_kernel reads them.  The module is walked in six 32-channel blocks j; stage j of the ring holds
// pw1's value and gate columns of block j (2 x 12 fragments) and the k rows 32 j .. 32 j + 31 of pw2 (6 x 2 fragments):
//     value, gate = pw1 xb (24 MFMAs)  ->  GLU, fp32, into an LDS block [128][32]        | barrier
//     depthwise conv + swish: thread = (channel, run of ceil(TR / 8) output rows), sliding window in registers,
//       16-bit result into the LDS block [TR][32] that is pw2's B operand                 | barrier
//     out[jo] += pw2[k block j][jo] dw (12 MFMAs, six 32-channel output blocks: k ascends with j, one chain per accumulator)
// and the epilogue adds bias and residual.  The GLU and depthwise blocks alias the window, which is dead once xb is loaded.
#include "common.h"
#include "conformer_ops.h"
#include "conv_epilogue.h"

namespace tts {

namespace {
constexpr int CC_C = 192;                       // model width
constexpr int CC_KS = CC_C / 16;                // k steps of a 192-channel contraction
constexpr int CC_J = CC_C / 32;                 // 32-channel blocks
constexpr int CC_ROWS = 128;                    // rows a workgroup normalises and multiplies
constexpr int CC_XP = CC_C + 8;                 // window pitch (16-bit elements): rows 16-byte aligned, conflict-free ds_read_b128
constexpr int CC_WIN = CC_ROWS * CC_XP * 2;     // 50 KB
constexpr int CC_FRAGS = 36;                    // fragments (1 KB) per stage
constexpr int CC_STAGE = CC_FRAGS * 1024;
constexpr int CC_GP = 36;                       // pitch of the fp32 GLU block (floats)
constexpr int CC_GLU = CC_ROWS * CC_GP * 4;     // 18 KB
constexpr int CC_DP = 40;                       // pitch of the 16-bit depthwise block (elements)
constexpr int CC_DWB = CC_ROWS * CC_DP * 2;     // 10 KB
constexpr int CC_CONST = CC_WIN + 2 * CC_STAGE; // byte offset of the constants behind the ring
constexpr int LQ_MAX_COUT = 1024;               // (one 16-byte unit of the bias per thread)
static_assert(CC_GLU + CC_DWB <= CC_WIN, "the GLU and depthwise blocks alias the window");
static_assert(CC_FRAGS % 4 == 0, "a stage splits evenly over the four wavefronts");

// (16-byte staging registers as ext-vectors: arrays of the uint4 / float4 structs were left in scratch memory)
typedef unsigned int cc_w128 __attribute__((ext_vector_type(4)));
constexpr int CC_WPL = CC_FRAGS / 4;            // 16-byte units of a stage per lane: wavefront w moves fragments 4 i + w

// An fp32 value that the replaced launches stored to memory, as the 16-bit operand the next product makes of it.  The value is
// pinned in a register first: otherwise the compiler folds the operation that produced it into the conversion (v_fma_mixlo_f16:
// one rounding, straight to fp16, where the stand-alone kernels round to fp32 and then to fp16) and the operand differs by an
// fp16 ulp in the double-rounding cases.
template <bool F16>
__device__ __forceinline__ unsigned short round16(float v) {
  TTS_PIN(v);
  return to16<F16>(v);
}

// LDS writes of every wavefront visible, every wavefront past its earlier LDS reads (global loads stay in flight: no __syncthreads)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// LayerNorm of this wavefront's 32 window rows (window row wr = packed row row_first + wr, clamped into [lo, hi)) into the window
template <bool F16>
__device__ __forceinline__ void ln_rows_to_window(const float* __restrict__ x, int ld_x, const float* __restrict__ g, const float* __restrict__ b,
                                                  float eps, int row_first, int lo, int hi, unsigned short* win, int wave, int lane) {
  // all 32 rows are requested before the first is used: one memory round trip (a row at a time it was 32 of them)
  constexpr int PL = CC_C / 64;
  float xv[32][PL];
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    int gr = row_first + wave * 32 + r;
    gr = gr < lo ? lo : (gr >= hi ? hi - 1 : gr);
#pragma unroll
    for (int i = 0; i < PL; ++i) xv[r][i] = x[(size_t)gr * ld_x + lane + 64 * i];
  }
  float gg[LN_MAX_PER_LANE], bb[LN_MAX_PER_LANE];
#pragma unroll
  for (int i = 0; i < LN_MAX_PER_LANE; ++i) {
    gg[i] = i < PL ? g[lane + 64 * (i < PL ? i : 0)] : 0.f;
    bb[i] = i < PL ? b[lane + 64 * (i < PL ? i : 0)] : 0.f;
  }
  __builtin_amdgcn_sched_barrier(0);  // (left to the scheduler the loads are sunk to their uses, eight at a time)
  constexpr int NR = 16;  // rows whose reductions run together
#pragma unroll
  for (int r0 = 0; r0 < 32; r0 += NR) {
    float v[NR][LN_MAX_PER_LANE], o[NR][LN_MAX_PER_LANE];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int i = 0; i < LN_MAX_PER_LANE; ++i) v[r][i] = i < PL ? xv[r0 + r][i < PL ? i : 0] : 0.f;
    layernorm_rows<NR>(v, lane, CC_C, eps, gg, bb, o);
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int i = 0; i < PL; ++i) win[(wave * 32 + r0 + r) * CC_XP + lane + 64 * i] = round16<F16>(o[r][i]);
  }
}

// the wavefront's rows back as B operands: lane = row, k step ks = channels 16 ks + 8 lk .. + 7
__device__ __forceinline__ void window_operands(const unsigned short* win, int wave, int lrow, int lk, bf16x8 (&xb)[CC_KS]) {
#pragma unroll
  for (int ks = 0; ks < CC_KS; ++ks) xb[ks] = *reinterpret_cast<const bf16x8*>(win + (wave * 32 + lrow) * CC_XP + ks * 16 + lk * 8);
}
}  // namespace

template <bool F16, int K>
__global__ __launch_bounds__(256, 1) void conformer_conv_kernel(const ConformerConv d) {
  constexpr int H = (K - 1) / 2, TR = CC_ROWS - (K - 1), DR = (TR + 7) / 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  unsigned short* win = reinterpret_cast<unsigned short*>(lds_raw);
  float* glu = reinterpret_cast<float*>(lds_raw);                               // [128][CC_GP]   (aliases the window)
  unsigned short* dwb = reinterpret_cast<unsigned short*>(lds_raw + CC_GLU);    // [128][CC_DP]   (aliases the window)
  unsigned char* ring = lds_raw + CC_WIN;                                       // [2][CC_STAGE]
  float* cb1 = reinterpret_cast<float*>(lds_raw + CC_CONST);                    // pw1 bias [value 192 | gate 192]
  float* cb2 = cb1 + 2 * CC_C;                                                  // pw2 bias
  float* cdb = cb2 + CC_C;                                                      // depthwise bias
  float* cdw = cdb + CC_C;                                                      // depthwise weights [K][192]
  const TtsTile tile = d.tiles[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lk = lane >> 5;
  const char* w1 = reinterpret_cast<const char*>(d.w1);
  const char* w2 = reinterpret_cast<const char*>(d.w2);

  // stage j: fragments 0 .. 11 pw1 value (k step = fragment), 12 .. 23 pw1 gate, 24 + 2 jo + ks2: pw2 rows 32 j + 16 ks2 .., columns 32 jo ..
  // a fragment's lane (lk, n) is the 16-byte unit (k / 8 = kb, column) of the packing; wavefront w moves fragments 4 i + w
  cc_w128 wreg[CC_WPL];
  auto fetch = [&](int j) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < CC_WPL; ++i) {
      const int f = 4 * i + wave;
      const char* src;
      if (i < 3) {
        src = w1 + ((size_t)(2 * f + lk) * d.w1_n + 32 * j + lrow) * 16;
      } else if (i < 6) {
        src = w1 + ((size_t)(2 * (f - 12) + lk) * d.w1_n + d.w1_half + 32 * j + lrow) * 16;
      } else {
        const int q = f - 24, jo = q >> 1, ks2 = q & 1;
        src = w2 + ((size_t)(4 * j + 2 * ks2 + lk) * d.w2_n + 32 * jo + lrow) * 16;
      }
      wreg[i] = *reinterpret_cast<const cc_w128*>(src);
    }
  };
  auto commit = [&](int j) __attribute__((always_inline)) {
    unsigned char* dst = ring + (size_t)(j & 1) * CC_STAGE + lane * 16;
#pragma unroll
    for (int i = 0; i < CC_WPL; ++i) *reinterpret_cast<cc_w128*>(dst + (size_t)(4 * i + wave) * 1024) = wreg[i];
  };
  fetch(0);

  {  // constants to LDS, 16 bytes at a time, every load in front of the first store: [b1 | b2 | dw_b] one unit per thread, dw_w NQ
    constexpr int NQ = (K * CC_C / 4 + 255) / 256;
    const int t = tid < CC_C ? tid : CC_C - 1;
    const float* s0 = t < 96 ? d.b1 + 4 * t : (t < 144 ? d.b2 + 4 * (t - 96) : d.dw_b + 4 * (t - 144));
    f32x4 cv[NQ + 1];
    cv[0] = *reinterpret_cast<const f32x4*>(s0);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int u = tid + 256 * q < K * CC_C / 4 ? tid + 256 * q : K * CC_C / 4 - 1;
      cv[1 + q] = *reinterpret_cast<const f32x4*>(d.dw_w + 4 * u);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (tid < CC_C) *reinterpret_cast<f32x4*>(cb1 + 4 * tid) = cv[0];  // (cb1 | cb2 | cdb are contiguous)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (tid + 256 * q < K * CC_C / 4) *reinterpret_cast<f32x4*>(cdw + 4 * (tid + 256 * q)) = cv[1 + q];
  }

  const int row_first = tile.row0 - H;  // packed row of window row 0
  ln_rows_to_window<F16>(d.x, d.ld_x, d.ln_g, d.ln_b, d.eps, row_first, tile.seq_begin, tile.seq_end, win, wave, lane);
  bf16x8 xb[CC_KS];
  window_operands(win, wave, lrow, lk, xb);  // (a wavefront reads the rows it wrote: no barrier)
  commit(0);

  TtsConvDesc e1 = {}, e2 = {};  // the fields epilogue_value reads
  e1.mode = TTS_MODE_GLU; e1.alpha = 1.0f;
  e2.mode = TTS_MODE_LINEAR; e2.act = TTS_ACT_NONE; e2.alpha = 1.0f; e2.res = d.x; e2.res_scale = 1.0f;

  f32x16 out[CC_J];
#pragma unroll
  for (int jo = 0; jo < CC_J; ++jo)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[jo][r] = 0.0f;

  const int wrow = wave * 32 + lrow;  // this lane's row: of the window in pw1, of the stored rows in pw2
  const bool in_seq = row_first + wrow >= tile.seq_begin && row_first + wrow < tile.seq_end;

  for (int j = 0; j < CC_J; ++j) {
    // stage j is there; every wavefront is past block j - 1 (its reads of the other stage and of the GLU / depthwise blocks; at
    // j = 0: past its reads of the window, and the constants are visible)
    lds_barrier();
    if (j + 1 < CC_J) fetch(j + 1);
    const unsigned char* st = ring + (size_t)(j & 1) * CC_STAGE + lane * 16;
    f32x16 av, ag;
#pragma unroll
    for (int r = 0; r < 16; ++r) av[r] = ag[r] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < CC_KS; ++ks) av = mfma16<F16>(*reinterpret_cast<const bf16x8*>(st + ks * 1024), xb[ks], av);
#pragma unroll
    for (int ks = 0; ks < CC_KS; ++ks) ag = mfma16<F16>(*reinterpret_cast<const bf16x8*>(st + (CC_KS + ks) * 1024), xb[ks], ag);
    // GLU: registers 4 rq + i = channels 32 j + 8 rq + 4 lk + i of the lane's row
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int n = 8 * rq + 4 * lk;
      const float4 ba = *reinterpret_cast<const float4*>(cb1 + 32 * j + n), bg = *reinterpret_cast<const float4*>(cb1 + CC_C + 32 * j + n);
      float4 v;
      v.x = epilogue_value<true>(e1, av[4 * rq + 0], ag[4 * rq + 0], ba.x, bg.x, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
      v.y = epilogue_value<true>(e1, av[4 * rq + 1], ag[4 * rq + 1], ba.y, bg.y, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
      v.z = epilogue_value<true>(e1, av[4 * rq + 2], ag[4 * rq + 2], ba.z, bg.z, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
      v.w = epilogue_value<true>(e1, av[4 * rq + 3], ag[4 * rq + 3], ba.w, bg.w, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
      if (!in_seq) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // zero padding of the depthwise conv
      *reinterpret_cast<float4*>(glu + wrow * CC_GP + n) = v;
    }
    lds_barrier();
    // depthwise conv + swish: stored row o reads window rows o .. o + K - 1
    {
      const int c = tid & 31, o0 = (tid >> 5) * DR;
      float wk[K];
#pragma unroll
      for (int t = 0; t < K; ++t) wk[t] = cdw[t * CC_C + 32 * j + c];
      const float bias = cdb[32 * j + c];
      float wv[DR + K - 1];
#pragma unroll
      for (int i = 0; i < DR + K - 1; ++i) {
        const int wr = o0 + i < CC_ROWS ? o0 + i : CC_ROWS - 1;  // (past the window: only stored rows >= TR would use it)
        wv[i] = glu[wr * CC_GP + c];
      }
#pragma unroll
      for (int i = 0; i < DR; ++i)
        if (o0 + i < TR) dwb[(o0 + i) * CC_DP + c] = round16<F16>(dwconv_swish_value(wk, wv, i, bias));
    }
    lds_barrier();
    {
      const unsigned short* dr = dwb + wrow * CC_DP + lk * 8;
      const bf16x8 h0 = *reinterpret_cast<const bf16x8*>(dr), h1 = *reinterpret_cast<const bf16x8*>(dr + 16);
#pragma unroll
      for (int jo = 0; jo < CC_J; ++jo) {
        out[jo] = mfma16<F16>(*reinterpret_cast<const bf16x8*>(st + (2 * CC_KS + 2 * jo) * 1024), h0, out[jo]);
        out[jo] = mfma16<F16>(*reinterpret_cast<const bf16x8*>(st + (2 * CC_KS + 2 * jo + 1) * 1024), h1, out[jo]);
      }
    }
    if (j + 1 < CC_J) commit(j + 1);  // (the other stage: last read in block j - 1, and every wavefront has passed a barrier since)
  }

  // ---- epilogue: bias and residual; lane = stored row wrow (rows TR .. 127 of the last wavefront are not stored)
  const int row = tile.row0 + wrow;
  const bool live = wrow < TR && row < tile.seq_end;
  const size_t rowc = live ? row : tile.row0;
  const float* xr = d.x + rowc * d.ld_x;
  float* yr = d.y + rowc * d.ld_y;
  f32x4 res[CC_J][4];  // (every residual read in front of the first store: one round trip)
#pragma unroll
  for (int jo = 0; jo < CC_J; ++jo)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) res[jo][rq] = *reinterpret_cast<const f32x4*>(xr + 32 * jo + 8 * rq + 4 * lk);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int jo = 0; jo < CC_J; ++jo)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      const int c = 32 * jo + 8 * rq + 4 * lk;
      const f32x4 rv = res[jo][rq];
      const float4 b = *reinterpret_cast<const float4*>(cb2 + c);
      float4 v;
      v.x = epilogue_value<false>(e2, out[jo][4 * rq + 0], 0.0f, b.x, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, rv.x);
      v.y = epilogue_value<false>(e2, out[jo][4 * rq + 1], 0.0f, b.y, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, rv.y);
      v.z = epilogue_value<false>(e2, out[jo][4 * rq + 2], 0.0f, b.z, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, rv.z);
      v.w = epilogue_value<false>(e2, out[jo][4 * rq + 3], 0.0f, b.w, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, rv.w);
      if (live) *reinterpret_cast<float4*>(yr + c) = v;
    }
}

// LayerNorm + 1-tap conv: stage s of the ring holds the columns 96 s .. 96 s + 95 (three 32-column blocks x 12 k steps)
template <bool F16>
__global__ __launch_bounds__(256, 1) void ln_linear_kernel(const LnLinear d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  unsigned short* win = reinterpret_cast<unsigned short*>(lds_raw);
  unsigned char* ring = lds_raw + CC_WIN;
  float* cb = reinterpret_cast<float*>(lds_raw + CC_CONST);  // bias [cout]
  const TtsTile tile = d.tiles[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lk = lane >> 5;
  const char* w = reinterpret_cast<const char*>(d.w);
  const int n_stages = d.cout / 96;

  cc_w128 wreg[CC_WPL];
  auto fetch = [&](int s) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < CC_WPL; ++i) {
      const int f = 4 * i + wave, blk = i / 3, ks = f - CC_KS * blk;  // (fragments 12 blk .. 12 blk + 11 belong to column block blk)
      wreg[i] = *reinterpret_cast<const cc_w128*>(w + ((size_t)(2 * ks + lk) * d.w_n + 96 * s + 32 * blk + lrow) * 16);
    }
  };
  auto commit = [&](int s) __attribute__((always_inline)) {
    unsigned char* dst = ring + (size_t)(s & 1) * CC_STAGE + lane * 16;
#pragma unroll
    for (int i = 0; i < CC_WPL; ++i) *reinterpret_cast<cc_w128*>(dst + (size_t)(4 * i + wave) * 1024) = wreg[i];
  };
  fetch(0);
  if (4 * tid < d.cout) *reinterpret_cast<float4*>(cb + 4 * tid) = *reinterpret_cast<const float4*>(d.bias + 4 * tid);

  ln_rows_to_window<F16>(d.x, d.ld_x, d.ln_g, d.ln_b, d.eps, tile.row0, tile.seq_begin, tile.seq_end, win, wave, lane);
  bf16x8 xb[CC_KS];
  window_operands(win, wave, lrow, lk, xb);
  commit(0);

  TtsConvDesc e = {};
  e.mode = TTS_MODE_LINEAR; e.act = TTS_ACT_NONE; e.alpha = 1.0f;
  const int row = tile.row0 + wave * 32 + lrow;
  const bool live = row < tile.seq_end;
  float* yr = d.y + (size_t)(live ? row : tile.row0) * d.ld_y;

  for (int s = 0; s < n_stages; ++s) {
    lds_barrier();  // stage s is there; everybody is past stage s - 1
    if (s + 1 < n_stages) fetch(s + 1);
    const unsigned char* st = ring + (size_t)(s & 1) * CC_STAGE + lane * 16;
    f32x16 acc[3];
#pragma unroll
    for (int blk = 0; blk < 3; ++blk) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[blk][r] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < CC_KS; ++ks) acc[blk] = mfma16<F16>(*reinterpret_cast<const bf16x8*>(st + (CC_KS * blk + ks) * 1024), xb[ks], acc[blk]);
    }
#pragma unroll
    for (int blk = 0; blk < 3; ++blk)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int c = 96 * s + 32 * blk + 8 * rq + 4 * lk;
        const float4 b = *reinterpret_cast<const float4*>(cb + c);
        float4 v;
        v.x = epilogue_value<false>(e, acc[blk][4 * rq + 0], 0.0f, b.x, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
        v.y = epilogue_value<false>(e, acc[blk][4 * rq + 1], 0.0f, b.y, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
        v.z = epilogue_value<false>(e, acc[blk][4 * rq + 2], 0.0f, b.z, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
        v.w = epilogue_value<false>(e, acc[blk][4 * rq + 3], 0.0f, b.w, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
        if (live) *reinterpret_cast<float4*>(yr + c) = v;
      }
    if (s + 1 < n_stages) commit(s + 1);
  }
}

int conformer_conv_tile_rows(int kernel) { return CC_ROWS - (kernel - 1); }

namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <class Kern, class Desc>
int launch_fused(const char* what, Kern kern, unsigned long long& raised, const Desc& d, size_t lds, hipStream_t st) {
  if (raise_lds_limit(reinterpret_cast<const void*>(kern), raised) != hipSuccess) {
    set_error("%s: raising the dynamic LDS limit failed", what);
    return TTS_E_LAUNCH;
  }
  hipLaunchKernelGGL(kern, dim3(d.n_tiles), dim3(256), lds, st, d);
  return launch_status(what);
}
}  // namespace

int conformer_conv(const ConformerConv& d, hipStream_t st) {
  TTS_CHECK_ARG(d.x && d.y && d.ln_g && d.ln_b && d.w1 && d.b1 && d.dw_w && d.dw_b && d.w2 && d.b2 && d.tiles, "conformer_conv: null pointer");
  TTS_CHECK_ARG(d.x != d.y, "conformer_conv: x cannot be updated in place (a workgroup reads its neighbours' rows as halo)");
  // (the kernel is written for any odd K <= 31 and gave the encoder's bits at K = 7 too, but the encoder measured slower fused
  // (DESIGN.md section 5, r10a), so only the decoder's size is built)
  TTS_CHECK_ARG(d.kernel == 31, "conformer_conv: kernel size %d unsupported (31)", d.kernel);
  TTS_CHECK_ARG(d.compute == TTS_COMPUTE_BF16 || d.compute == TTS_COMPUTE_F16, "conformer_conv: 16-bit MFMA configurations only (compute %d)", d.compute);
  TTS_CHECK_ARG(d.tile_rows == conformer_conv_tile_rows(d.kernel), "conformer_conv: tile table must use %d rows, got %d", conformer_conv_tile_rows(d.kernel), d.tile_rows);
  TTS_CHECK_ARG(d.w1_half >= CC_C && d.w1_n >= d.w1_half + CC_C && d.w2_n >= CC_C, "conformer_conv: packed widths %d (gate from %d) / %d are below the model width", d.w1_n, d.w1_half, d.w2_n);
  TTS_CHECK_ARG(d.ld_x >= CC_C && d.ld_y >= CC_C && (d.ld_x & 3) == 0 && (d.ld_y & 3) == 0 && aligned16(d.x) && aligned16(d.y) && aligned16(d.w1) && aligned16(d.w2) &&
                    aligned16(d.b1) && aligned16(d.b2) && aligned16(d.dw_w) && aligned16(d.dw_b),
                "conformer_conv: rows, weights and biases must be 16-byte aligned");
  if (d.n_tiles <= 0) return TTS_OK;
  const bool f16 = d.compute == TTS_COMPUTE_F16;
  const size_t lds = CC_CONST + (size_t)(4 * CC_C + d.kernel * CC_C) * sizeof(float);
  static unsigned long long raised[2] = {0, 0};
  if (f16) return launch_fused("conformer_conv", conformer_conv_kernel<true, 31>, raised[0], d, lds, st);
  return launch_fused("conformer_conv", conformer_conv_kernel<false, 31>, raised[1], d, lds, st);
}

int ln_linear(const LnLinear& d, hipStream_t st) {
  TTS_CHECK_ARG(d.x && d.y && d.ln_g && d.ln_b && d.w && d.bias && d.tiles, "ln_linear: null pointer");
  TTS_CHECK_ARG(d.compute == TTS_COMPUTE_BF16 || d.compute == TTS_COMPUTE_F16, "ln_linear: 16-bit MFMA configurations only (compute %d)", d.compute);
  TTS_CHECK_ARG(d.tile_rows == CC_ROWS, "ln_linear: tile table must use %d rows, got %d", CC_ROWS, d.tile_rows);
  TTS_CHECK_ARG(d.cout >= 96 && d.cout % 96 == 0 && d.cout <= LQ_MAX_COUT && d.w_n >= d.cout, "ln_linear: %d output channels (%d packed) unsupported: a multiple of 96 up to %d",
                d.cout, d.w_n, LQ_MAX_COUT);
  TTS_CHECK_ARG(d.ld_x >= CC_C && d.ld_y >= d.cout && (d.ld_y & 3) == 0 && aligned16(d.y) && aligned16(d.w) && aligned16(d.bias), "ln_linear: rows, weights and bias must be 16-byte aligned");
  if (d.n_tiles <= 0) return TTS_OK;
  const bool f16 = d.compute == TTS_COMPUTE_F16;
  const size_t lds = CC_CONST + (size_t)d.cout * sizeof(float);
  static unsigned long long raised[2] = {0, 0};
  if (f16) return launch_fused("ln_linear", ln_linear_kernel<true>, raised[0], d, lds, st);
  return launch_fused("ln_linear", ln_linear_kernel<false>, raised[1], d, lds, st);
}

}  // namespace tts
