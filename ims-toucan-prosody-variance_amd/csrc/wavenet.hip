// One WaveNet layer of the PostFlow's coupling blocks in one launch (16-bit MFMA configurations):
//   acts = tanh(a) * sigmoid(g),  [a | g] = in_layer(h) (5 taps, 192 -> 384) + bias + cond          wavenet.py:104-110, :29-35
//   [h | skip] += res_skip_layer(acts) (1 tap, 192 -> 384; last layer: 192 -> 192 into the skip sum)   wavenet.py:112-118
// Two launches (tts_conv1d in GATED mode, then an accumulating 1-tap conv) cost 37 + 29 us per layer at batch 32 - 72 layers per
// pass - almost all of it fixed per-launch / per-slab latency on tiny GEMMs (K = 192).  Here one 256-thread workgroup owns 64
// frames of one utterance and ALL output channels: the gate activations never leave LDS and the hidden state is read and
// written once.  Because a 5-tap conv reads two frames either side of the tile, the hidden state cannot be updated in place:
// the layer reads hs_in and writes hs_out (the host ping-pongs two buffers).
//
// Both products run transposed (weights are the MFMA A operand, accumulator row = output channel, lane = frame), so epilogues
// work on float4 / packed 8-byte pieces of a frame's row (see resblock.hip).
//
// No wavefront waits for another inside a product.  Every wavefront streams the weight columns it consumes itself straight from
// global memory (L2) into registers as A fragments - the packed layout [tap][k/8][n][8] makes a fragment one coalesced
// global_load_dwordx4 - WN_DEPTH k-steps ahead with counted s_waitcnt vmcnt, as gemm_rows_kernel in conv1d.hip does; only the
// hidden-state window, and later acts, are shared in LDS.  Three barriers per layer: the window is staged; every wave is done
// with it; acts are complete.  (The predecessor streamed 24 KB weight slabs through an LDS ring shared by the four wavefronts,
// one barrier per slab: 36 dependent steps of ~0.9 us, neither the loads nor the MFMAs but that chain set its 32 us.)
// Ownership: the gated conv is 12 work items (pair-block of 32 a + 32 g channels, frame block of 32), three per wavefront - one
// pair-block over both frame blocks (each fragment feeds two MFMAs) and half of a pair-block shared with the neighbouring
// wavefront: 4 fragments and 6 MFMAs per k-step, L2 -> CU weight traffic 8/6 of the matrix.  The res/skip conv gives a wavefront
// three output-channel blocks over both frame blocks (last layer: the gated conv's pattern on its six blocks).
// Accumulation order of both products is the predecessor's: tap-major, k ascending in 16-channel steps.
//
// Fused conditioning (wavenet_layer_cond, the PostFlow of the stage API): the block's cond conv (1 tap, 384 -> 1536) used to
// write [rows, 1536] fp32 that the four layers read back in 384-column slices - 2.3 GB of HBM traffic per pass for a value used
// once.  Here the layer computes its own 384 columns as a third product in the same stream, from a 16-bit LDS tile of the
// squeezed g, into accumulators of its own and in the arithmetic of tts_conv1d's 16-bit loop (32x32x16, k ascending,
// (acc + bias) in fp32), so the result is bit-identical to the two-launch form that engine.py keeps.
#include "common.h"

namespace tts {

namespace {
constexpr int WN_H = 192;           // hidden channels
constexpr int WN_BM = 64;            // frames per workgroup
constexpr int WN_TAPS = 5;
constexpr int WN_XP = WN_H + 8;      // LDS pitch of the window / of acts (16-bit elements)
constexpr int WN_G = 2 * WN_H;       // channels of the squeezed g (fused conditioning)
constexpr int WN_GP = WN_G + 8;      // LDS pitch of the g tile
constexpr int WN_STEPS1 = WN_TAPS * (WN_H / 16);  // 60 k-steps of the gated conv
constexpr int WN_STEPSC = WN_G / 16;              // 24 of the conditioning conv
constexpr int WN_STEPS2 = WN_H / 16;              // 12 of the res/skip conv
constexpr int WN_DEPTH = 4;          // k-steps of weight fragments in flight per wavefront (divides 12; six spill the fused form)
constexpr int WN_L = 4;              // loads per wavefront and k-step, in every product (the res/skip one pads with a repeat)
constexpr size_t WN_XS_BYTES = ((size_t)(WN_BM + WN_TAPS - 1) * WN_XP * 2 + 255) / 256 * 256;
constexpr size_t WN_GS_BYTES = (size_t)WN_BM * WN_GP * 2;
static_assert(WN_STEPS1 % WN_DEPTH == 0 && WN_STEPSC % WN_DEPTH == 0 && WN_STEPS2 % WN_DEPTH == 0 && (WN_H / 16) % WN_DEPTH == 0,
              "a block of WN_DEPTH k-steps stays inside one tap and one product");
}  // namespace

template <bool F16, bool FUSED>
__global__ __launch_bounds__(256) void wavenet_layer_kernel(const TtsWavenetDesc d, const WavenetCond cd) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  unsigned short* xs = reinterpret_cast<unsigned short*>(lds_raw);                // [68][XP] window of h, later [64][XP] acts
  unsigned short* gs = reinterpret_cast<unsigned short*>(lds_raw + WN_XS_BYTES);  // FUSED: [64][GP] squeezed g, 16-bit
  const TtsTile tile = d.tiles[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, lrow = lane & 31, lk = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // ownership: pair-block P0 (32 a + 32 g channels) over both frame blocks, pair-block P1 over frame block fP only
  const int P0 = (wave * 5 + 1) / 3, P1 = wave < 2 ? 1 : 4, fP = wave & 1, fQ = fP ^ 1;  // P0 = 0, 2, 3, 5
  const int n2 = d.cout2;  // 384 or 192
  // res/skip: output-channel blocks 3 wave .. 3 wave + 2 over both frame blocks; the last layer (six blocks): P0 over both, P1 over fP
  const int cb0 = n2 == 384 ? 3 * wave : P0, cb1 = n2 == 384 ? 3 * wave + 1 : P1, cb2 = n2 == 384 ? 3 * wave + 2 : P1;

  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  // The weight stream (see TTS_GLOAD128 in common.h for the idiom): inline-asm loads the compiler does not count, WN_DEPTH
  // k-steps ahead; they return in order, so before a k-step is consumed (WN_DEPTH - 1) * WN_L younger loads may stay in flight.
  // One stream runs through all products: the last block of a product requests the first k-steps of the next one.
  u32x4 wr[WN_DEPTH][WN_L];
  const char *q0, *q1, *q2, *q3;  // this lane's four fragment addresses of the next k-step to request
  size_t qs;                      // bytes per k-step
  auto request = [&](int slot) __attribute__((always_inline)) {
    TTS_GLOAD128(wr[slot][0], q0);
    TTS_GLOAD128(wr[slot][1], q1);
    TTS_GLOAD128(wr[slot][2], q2);
    TTS_GLOAD128(wr[slot][3], q3);
    q0 += qs; q1 += qs; q2 += qs; q3 += qs;
  };
  auto arrive = [&](int slot) __attribute__((always_inline)) {
    TTS_WAIT_VM((WN_DEPTH - 1) * WN_L);
    TTS_PIN(wr[slot][0]);
    TTS_PIN(wr[slot][1]);
    TTS_PIN(wr[slot][2]);
    TTS_PIN(wr[slot][3]);
  };
  // packed [tap][k/8][n][8]: the A fragment of k-step s, column block cb = 16 bytes at ((2 s + lk) n + 32 cb + lrow) * 16
  auto stream_pairs = [&](const void* w, int n, int col0) __attribute__((always_inline)) {  // columns a | g of P0 and of P1
    const char* b = reinterpret_cast<const char*>(w) + ((size_t)lk * n + col0 + lrow) * 16;
    q0 = b + P0 * 512; q1 = q0 + WN_H * 16; q2 = b + P1 * 512; q3 = q2 + WN_H * 16;
    qs = (size_t)n * 32;
  };
  auto stream_res_skip = [&]() __attribute__((always_inline)) {
    const char* b = reinterpret_cast<const char*>(d.w2) + ((size_t)lk * n2 + lrow) * 16;
    q0 = b + cb0 * 512; q1 = b + cb1 * 512; q2 = b + cb2 * 512; q3 = q2;
    qs = (size_t)n2 * 32;
  };
  auto publish = [&]() __attribute__((always_inline)) {  // this wave's LDS stores are done, then the barrier (raw: no vmcnt drain)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  // ---- FUSED: this thread's share of the tile's g rows (rows past the utterance read its last row: their results are never
  // stored).  Requested first and parked in accumulator registers until the gated conv's loop is over: the loads return in order,
  // so the waits of the window staging below cover them and no wait of the weight stream ever meets them in flight.
  constexpr int GQ4 = WN_G / 4, GPER = WN_BM * GQ4 / 256;  // 24 float4 per thread
  f32x4 gv[FUSED ? GPER : 1];
  if constexpr (FUSED) {
#pragma unroll
    for (int p = 0; p < GPER; ++p) {
      const int e = tid + p * 256, r = e / GQ4, c4 = (e % GQ4) * 4;
      int gr = tile.row0 + r;
      gr = gr < tile.seq_end ? gr : tile.seq_end - 1;
      const float* gp = cd.g + (size_t)gr * cd.ld_g + c4;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(gv[p]) : "v"(gp) : "memory");
    }
  }
  stream_pairs(d.w1, 2 * WN_H, 0);
#pragma unroll
  for (int u = 0; u < WN_DEPTH; ++u) request(u);  // the first fragments land while the window is staged

  // ---- window of the hidden state: rows row0 - 2 .. row0 + 65 (zero outside the utterance = the conv's zero padding) -> 16-bit
  {
    // PER independent 16-byte loads per thread are in flight before the first is consumed (clamped addresses, no branches): one
    // trip pays the HBM latency once, not once per load
    constexpr int Q4 = WN_H / 4, ROWS = WN_BM + WN_TAPS - 1, TOTAL = ROWS * Q4, PER = 7;
    for (int base = tid; base < TOTAL; base += 256 * PER) {
      float4 v[PER];
#pragma unroll
      for (int p = 0; p < PER; ++p) {
        int e = base + p * 256;
        e = e < TOTAL ? e : TOTAL - 1;
        const int r = e / Q4, c4 = (e % Q4) * 4;
        const int gr = tile.row0 - 2 + r;
        const int grc = gr < tile.seq_begin ? tile.seq_begin : (gr >= tile.seq_end ? tile.seq_end - 1 : gr);
        v[p] = *reinterpret_cast<const float4*>(d.hs_in + (size_t)grc * d.ld_in + c4);
        if (gr != grc) v[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int p = 0; p < PER; ++p) {
        const int e = base + p * 256;
        if (e < TOTAL) {
          const int r = e / Q4, c4 = (e % Q4) * 4;
          *reinterpret_cast<uint2*>(xs + r * WN_XP + c4) = make_uint2(pack16<F16>(v[p].x, v[p].y), pack16<F16>(v[p].z, v[p].w));
        }
      }
    }
  }
  publish();  // (1) the window is staged

  f32x16 acc[6], accc[FUSED ? 6 : 1];
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

  // one k-step of a pair product: a[0..3] = P0's a (fP, fQ) and g (fP, fQ), a[4..5] = P1's a and g (fP).  xP / xQ hold this
  // k-step's frame fragments; the next k-step's (at xnext) are read before the MFMAs, so their LDS round trip hides under them
  auto xload = [&](bf16x8& xP, bf16x8& xQ, const unsigned short* xrow, int pitch) __attribute__((always_inline)) {
    xP = *reinterpret_cast<const bf16x8*>(xrow + (fP * 32 + lrow) * pitch + lk * 8);
    xQ = *reinterpret_cast<const bf16x8*>(xrow + (fQ * 32 + lrow) * pitch + lk * 8);
  };
  auto pair_step = [&](int slot, f32x16 (&a)[6], bf16x8& xP, bf16x8& xQ, const unsigned short* xnext, int pitch) __attribute__((always_inline)) {
    const bf16x8 cP = xP, cQ = xQ;
    xload(xP, xQ, xnext, pitch);
    arrive(slot);
    u32x4 wf[WN_L];
#pragma unroll
    for (int i = 0; i < WN_L; ++i) wf[i] = wr[slot][i];  // copies: the slot is re-requested below while the MFMAs may still read
    a[0] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[0]), cP, a[0]);
    a[1] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[0]), cQ, a[1]);
    a[2] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[1]), cP, a[2]);
    a[3] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[1]), cQ, a[3]);
    a[4] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[2]), cP, a[4]);
    a[5] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[3]), cP, a[5]);
    request(slot);
  };
  bf16x8 xP, xQ;
  auto window_at = [&](int s) __attribute__((always_inline)) {  // k-step s of the gated conv: tap s / 12, channels 16 (s % 12) ..
    s = s < WN_STEPS1 ? s : WN_STEPS1 - 1;
    return xs + (s / (WN_H / 16)) * WN_XP + (s % (WN_H / 16)) * 16;
  };

  // ---- gated conv: tap-major, k ascending in 16-channel steps
  xload(xP, xQ, window_at(0), WN_XP);
#pragma unroll 1
  for (int base = 0; base < WN_STEPS1; base += WN_DEPTH) {
    if (base == WN_STEPS1 - WN_DEPTH) {  // the requests of this block are the first k-steps of the next product
      if constexpr (FUSED) stream_pairs(cd.wc, cd.wc_n, cd.col0);
      else stream_res_skip();
    }
#pragma unroll
    for (int u = 0; u < WN_DEPTH; ++u) pair_step(u, acc, xP, xQ, window_at(base + u + 1), WN_XP);
  }
  // ---- FUSED: cond = cond_conv(g)[this layer's 384 columns] into its own accumulators (1 tap, K = 384, k ascending: the
  // arithmetic of the stand-alone conv, so acts are bit-identical to the two-launch form)
  if constexpr (FUSED) {
#pragma unroll
    for (int p = 0; p < GPER; ++p) {
      asm volatile("" : "+a"(gv[p]));  // (landed: older than every weight fragment consumed so far; no use moves above this)
      const int e = tid + p * 256, r = e / GQ4, c4 = (e % GQ4) * 4;
      *reinterpret_cast<uint2*>(gs + r * WN_GP + c4) = make_uint2(pack16<F16>(gv[p][0], gv[p][1]), pack16<F16>(gv[p][2], gv[p][3]));
    }
  }
  publish();  // (2) every wave is done reading the window (and g is staged)
  if constexpr (FUSED) {
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) accc[j][r] = 0.0f;
    xload(xP, xQ, gs, WN_GP);
#pragma unroll 1
    for (int base = 0; base < WN_STEPSC; base += WN_DEPTH) {
      if (base == WN_STEPSC - WN_DEPTH) stream_res_skip();
#pragma unroll
      for (int u = 0; u < WN_DEPTH; ++u) {
        const int s1 = base + u + 1 < WN_STEPSC ? base + u + 1 : WN_STEPSC - 1;
        pair_step(u, accc, xP, xQ, gs + s1 * 16, WN_GP);
      }
    }
  }
  // ---- acts = tanh(a + bias + cond) * sigmoid(g + bias + cond) -> LDS (over the window), 16-bit
  {
    auto gate = [&](const f32x16& aa, const f32x16& ag, const f32x16& ca, const f32x16& cg, int pb, int f) __attribute__((always_inline)) {
      const int t = f * 32 + lrow, row = tile.row0 + t;
      const float* cr = FUSED ? nullptr : d.cond + (size_t)(row < tile.seq_end ? row : tile.seq_end - 1) * d.ld_cond;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int c = pb * 32 + 8 * rq + 4 * lk;
        const float4 ba = *reinterpret_cast<const float4*>(d.b1 + c), bg = *reinterpret_cast<const float4*>(d.b1 + WN_H + c);
        float pa[4], pg[4];
        if constexpr (FUSED) {
          const float4 ea = *reinterpret_cast<const float4*>(cd.bc + cd.col0 + c), eg = *reinterpret_cast<const float4*>(cd.bc + cd.col0 + WN_H + c);
          const float eav[4] = {ea.x, ea.y, ea.z, ea.w}, egv[4] = {eg.x, eg.y, eg.z, eg.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // what the stand-alone conv's epilogue stores: (acc + bias + 0) * 1
            pa[q] = (ca[4 * rq + q] + eav[q]) + 0.0f;
            pg[q] = (cg[4 * rq + q] + egv[q]) + 0.0f;
          }
        } else {
          const float4 ea = *reinterpret_cast<const float4*>(cr + c), eg = *reinterpret_cast<const float4*>(cr + WN_H + c);
          pa[0] = ea.x; pa[1] = ea.y; pa[2] = ea.z; pa[3] = ea.w;
          pg[0] = eg.x; pg[1] = eg.y; pg[2] = eg.z; pg[3] = eg.w;
        }
        const float bav[4] = {ba.x, ba.y, ba.z, ba.w}, bgv[4] = {bg.x, bg.y, bg.z, bg.w};
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float av = aa[4 * rq + q] + bav[q] + pa[q], gvv = ag[4 * rq + q] + bgv[q] + pg[q];
          // hardware exp / reciprocal (a few ulp of 1 + e^-2a: tanh carries an ABSOLUTE error of about 2^-24, far below the 16-bit
          // rounding of acts for |a| above 2^-14 and above it below - the rounding model's option fast_gate, tests/abi_emulator.py;
          // DESIGN.md section 4, "The 16-bit kernels over the dynamic range"): with one wavefront per SIMD the library tanhf /
          // expf / IEEE division of 48 elements per lane were 6 us of a 37 us launch
          const float th = 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * av)) - 1.0f;
          v[q] = th * __builtin_amdgcn_rcpf(1.0f + __expf(-gvv));
        }
        *reinterpret_cast<uint2*>(xs + t * WN_XP + c) = make_uint2(pack16<F16>(v[0], v[1]), pack16<F16>(v[2], v[3]));
      }
    };
    constexpr int CZ = FUSED ? 1 : 0;  // (not FUSED: accc is one unused register block)
    gate(acc[0], acc[2], accc[0 * CZ], accc[2 * CZ], P0, fP);
    gate(acc[1], acc[3], accc[1 * CZ], accc[3 * CZ], P0, fQ);
    gate(acc[4], acc[5], accc[4 * CZ], accc[5 * CZ], P1, fP);
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
  }
  publish();  // (3) acts are complete
  // ---- res / skip conv: acc[2 i] = block cb_i over fP, acc[2 i + 1] over fQ (last layer: acc[0..2] only)
  xload(xP, xQ, xs, WN_XP);
#pragma unroll 1
  for (int base = 0; base < WN_STEPS2; base += WN_DEPTH) {
    if (base == WN_STEPS2 - WN_DEPTH) {  // nothing follows: the tail re-requests the last k-step (unused), no branch in the stream
      q0 -= qs; q1 -= qs; q2 -= qs; q3 -= qs;
      qs = 0;
    }
#pragma unroll
    for (int u = 0; u < WN_DEPTH; ++u) {
      const bf16x8 cP = xP, cQ = xQ;
      const int s1 = base + u + 1 < WN_STEPS2 ? base + u + 1 : WN_STEPS2 - 1;
      xload(xP, xQ, xs + s1 * 16, WN_XP);
      arrive(u);
      u32x4 wf[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) wf[i] = wr[u][i];
      acc[0] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[0]), cP, acc[0]);
      acc[1] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[0]), cQ, acc[1]);
      acc[2] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[1]), cP, acc[2]);
      if (n2 == 384) {
        acc[3] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[1]), cQ, acc[3]);
        acc[4] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[2]), cP, acc[4]);
        acc[5] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[2]), cQ, acc[5]);
      }
      request(u);
    }
  }
  TTS_WAIT_VM(0);  // drain the tail requests: their destination registers stay allocated (pinned) until here
#pragma unroll
  for (int u = 0; u < WN_DEPTH; ++u) {
    TTS_PIN(wr[u][0]);
    TTS_PIN(wr[u][1]);
    TTS_PIN(wr[u][2]);
    TTS_PIN(wr[u][3]);
  }
  // ---- [h | skip] out = in + res_skip + bias (last layer: the skip half only)
  {
    const int col0 = n2 == 384 ? 0 : WN_H;
    auto store_block = [&](const f32x16& a, int cb, int f) __attribute__((always_inline)) {
      const int row = tile.row0 + f * 32 + lrow;
      if (row >= tile.seq_end) return;
      const float* ir = d.hs_in + (size_t)row * d.ld_in + col0;
      float* orow = d.hs_out + (size_t)row * d.ld_out + col0;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int c = cb * 32 + 8 * rq + 4 * lk;
        const float4 b = *reinterpret_cast<const float4*>(d.b2 + c), x = *reinterpret_cast<const float4*>(ir + c);
        *reinterpret_cast<float4*>(orow + c) = make_float4((a[4 * rq] + b.x) + x.x, (a[4 * rq + 1] + b.y) + x.y, (a[4 * rq + 2] + b.z) + x.z, (a[4 * rq + 3] + b.w) + x.w);
      }
    };
    store_block(acc[0], cb0, fP);
    store_block(acc[1], cb0, fQ);
    store_block(acc[2], cb1, fP);
    if (n2 == 384) {
      store_block(acc[3], cb1, fQ);
      store_block(acc[4], cb2, fP);
      store_block(acc[5], cb2, fQ);
    }
  }
}

// ---- One coupling block (the start conv, the four WaveNet layers, end conv + coupling, inverse 1x1 conv + ActNorm) in one launch --
// h = start(x0) is computed in the workgroup (80 -> 192, five k-steps), then the layer body above, looped: the hidden state and the skip sum stay in the registers of the wavefronts that own their output
// channels in the res/skip product (waves 0, 1: h; waves 2, 3: skip), the next layer's 16-bit window is written straight from
// the res/skip epilogue, the squeezed g is staged once for the four conditioning products, and the weight stream runs on from
// one layer into the next.  The skip sum is not written either: the tail (below the layer loop) turns it into the block's new x,
// the only thing the launch writes, into a buffer of its own (x_out), since neighbours read the old x0.  Halo by recomputation: a workgroup computes the 64 rows
// row0 - 8 .. row0 + 55 through all four layers (each 5-tap layer costs 2 rows a side) and stores the central 48; the tile table
// has 48-row tiles.  In every layer's window the rows outside the utterance are zeros (the per-layer form's zero padding), also
// where they lie inside the computed range.  Acts have a buffer of their own, so a layer needs two barriers: the window is
// complete; acts are complete.  Every product keeps the per-layer kernel's k order and epilogue expressions: same bits.
// The last layer (192 res/skip columns) keeps the ownership of the others - waves 2, 3 own the skip blocks, waves 0, 1 repeat
// them and drop the result - so the skip sum never changes registers.
namespace {
constexpr int WB_OUT = 48;   // rows stored per workgroup
constexpr int WB_HALO = 8;   // 4 layers x 2 rows
constexpr int WB_CIN = 80;   // channels of x0, the start conv's input
constexpr int WB_COUT = 80;  // channels of x1 = of m and of logs, the halves of the end conv
constexpr int WB_X = 2 * WB_COUT;  // channels of x
constexpr int WB_MIXG = WB_X / 4;  // mixing groups of a row
constexpr int WB_SP = WN_H + 4;    // LDS pitch of the fp32 skip sum (floats): rows 4 banks apart, a 16-lane ds_read_b128 phase is conflict-free
constexpr size_t WB_AS_BYTES = (size_t)WN_BM * WN_XP * 2;
constexpr size_t WB_LDS_BYTES = WN_XS_BYTES + WN_GS_BYTES + WB_AS_BYTES;
static_assert(WB_OUT + 2 * WB_HALO == WN_BM, "stored rows plus the halo are the computed tile");
static_assert(((size_t)WN_BM * WB_SP + 3 * WB_X) * 4 <= WN_XS_BYTES + WN_GS_BYTES, "the fp32 skip sum and the epilogue's operands fit over the window and the g tile");
}  // namespace

template <bool F16>
__global__ __launch_bounds__(256) void wavenet_block_kernel(const WavenetBlock d) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  unsigned short* xs = reinterpret_cast<unsigned short*>(lds_raw);                               // [68][XP] window of h
  unsigned short* gs = reinterpret_cast<unsigned short*>(lds_raw + WN_XS_BYTES);                 // [64][GP] squeezed g
  unsigned short* as = reinterpret_cast<unsigned short*>(lds_raw + WN_XS_BYTES + WN_GS_BYTES);  // [64][XP] acts
  float* sk = reinterpret_cast<float*>(lds_raw);  // the tail: [64][SP] fp32 skip sum, over the window and g (nobody reads them then)
  const int tid = threadIdx.x, lane = tid & 63, lrow = lane & 31, lk = lane >> 5;
  // ---- workgroups behind the tile table: the rows of x that belong to no tile.  No coupling reaches them; they pass the inverse
  // 1x1 conv and ActNorm like every row (glow_mix_kernel's loop, reading x and writing x_out)
  if ((int)blockIdx.x >= d.n_tiles) {
    float w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = d.winv[i];
    const int total = d.n_pad * WB_MIXG;
    for (int e = ((int)blockIdx.x - d.n_tiles) * 256 + tid; e < total; e += ((int)gridDim.x - d.n_tiles) * 256) {
      const int r = d.pad_rows[e / WB_MIXG], g = e % WB_MIXG;
      const float* xr = d.x + (size_t)r * d.ld_x;
      float* orow = d.x_out + (size_t)r * d.ld_out;
      const int idx[4] = {2 * g, 2 * g + 1, WB_COUT + 2 * g, WB_COUT + 2 * g + 1};
      const float v0 = xr[idx[0]], v1 = xr[idx[1]], v2 = xr[idx[2]], v3 = xr[idx[3]];
#pragma unroll
      for (int o = 0; o < 4; ++o) orow[idx[o]] = glow_mix_value(w, o, v0, v1, v2, v3, d.an_bias[idx[o]], glow_actnorm_scale(d.an_logs[idx[o]]));
    }
    return;
  }
  const TtsTile tile = d.tiles[blockIdx.x];
  const int c0 = tile.row0 - WB_HALO;  // first computed row
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int P0 = (wave * 5 + 1) / 3, P1 = wave < 2 ? 1 : 4, fP = wave & 1, fQ = fP ^ 1;
  auto clamp_row = [&](int gr) __attribute__((always_inline)) { return gr < tile.seq_begin ? tile.seq_begin : (gr >= tile.seq_end ? tile.seq_end - 1 : gr); };
  auto pick = [&](auto (&arr)[4], int i) __attribute__((always_inline)) { return i == 0 ? arr[0] : (i == 1 ? arr[1] : (i == 2 ? arr[2] : arr[3])); };

  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  u32x4 wr[WN_DEPTH][WN_L];  // the weight stream of wavenet_layer_kernel
  const char *q0, *q1, *q2, *q3;
  size_t qs;
  auto request = [&](int slot) __attribute__((always_inline)) {
    TTS_GLOAD128(wr[slot][0], q0);
    TTS_GLOAD128(wr[slot][1], q1);
    TTS_GLOAD128(wr[slot][2], q2);
    TTS_GLOAD128(wr[slot][3], q3);
    q0 += qs; q1 += qs; q2 += qs; q3 += qs;
  };
  auto arrive = [&](int slot) __attribute__((always_inline)) {
    TTS_WAIT_VM((WN_DEPTH - 1) * WN_L);
    TTS_PIN(wr[slot][0]);
    TTS_PIN(wr[slot][1]);
    TTS_PIN(wr[slot][2]);
    TTS_PIN(wr[slot][3]);
  };
  auto stream_pairs = [&](const void* w, int n, int col0) __attribute__((always_inline)) {
    const char* b = reinterpret_cast<const char*>(w) + ((size_t)lk * n + col0 + lrow) * 16;
    q0 = b + P0 * 512; q1 = q0 + WN_H * 16; q2 = b + P1 * 512; q3 = q2 + WN_H * 16;
    qs = (size_t)n * 32;
  };
  auto stream_res_skip = [&](const void* w, int n, int cb) __attribute__((always_inline)) {  // blocks cb .. cb + 2
    const char* b = reinterpret_cast<const char*>(w) + ((size_t)lk * n + lrow) * 16 + cb * 512;
    q0 = b; q1 = b + 512; q2 = b + 1024; q3 = q2;
    qs = (size_t)n * 32;
  };
  auto publish = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  stream_pairs(d.w1[0], 2 * WN_H, 0);
#pragma unroll
  for (int u = 0; u < WN_DEPTH; ++u) request(u);

  // ---- the tile's g rows -> 16-bit, once for the four layers (rows outside the utterance read its nearest row: their results
  // are never stored)
  {
    constexpr int GQ4 = WN_G / 4, GPER = WN_BM * GQ4 / 256, PER = 8;
    static_assert(GPER % PER == 0, "g staging trips");
#pragma unroll 1
    for (int p0 = 0; p0 < GPER; p0 += PER) {
      float4 v[PER];
#pragma unroll
      for (int p = 0; p < PER; ++p) {
        const int e = tid + (p0 + p) * 256, r = e / GQ4, c4 = (e % GQ4) * 4;
        v[p] = *reinterpret_cast<const float4*>(d.g + (size_t)clamp_row(c0 + r) * d.ld_g + c4);
      }
#pragma unroll
      for (int p = 0; p < PER; ++p) {
        const int e = tid + (p0 + p) * 256, r = e / GQ4, c4 = (e % GQ4) * 4;
        *reinterpret_cast<uint2*>(gs + r * WN_GP + c4) = make_uint2(pack16<F16>(v[p].x, v[p].y), pack16<F16>(v[p].z, v[p].w));
      }
    }
  }
  // ---- h = start(x0) for the 64 computed rows, in the arithmetic of the stand-alone conv (16-bit 32x32x16, k ascending over the
  // 80 channels of x0, (acc + bias) + 0): waves 0, 1 compute the blocks they own in the res/skip product straight into the state
  // registers and write the first layer's window (zero outside the utterance).  Window rows 0, 1, 66, 67 reach no stored row
  // (the halo is 8 rows for the layers' 2 + 2 + 2 + 2): zeros.
  // The state: st[2 i] = res/skip block 3 wave + i over frame block fP, st[2 i + 1] over fQ.  Waves 0, 1: h in fp32 (the residual
  // input of every layer); waves 2, 3: the skip sum, which starts at zero.
  f32x16 st[6];
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) st[j][r] = 0.0f;
  if (wave < 2) {
    const float* xrP = d.x + (size_t)clamp_row(c0 + fP * 32 + lrow) * d.ld_x + lk * 8;
    const float* xrQ = d.x + (size_t)clamp_row(c0 + fQ * 32 + lrow) * d.ld_x + lk * 8;
    const char* wb = reinterpret_cast<const char*>(d.w0) + ((size_t)lk * d.w0_n + 96 * wave + lrow) * 16;
#pragma unroll
    for (int s = 0; s < WB_CIN / 16; ++s) {
      const float4 p0 = *reinterpret_cast<const float4*>(xrP + 16 * s), p1 = *reinterpret_cast<const float4*>(xrP + 16 * s + 4);
      const float4 r0 = *reinterpret_cast<const float4*>(xrQ + 16 * s), r1 = *reinterpret_cast<const float4*>(xrQ + 16 * s + 4);
      const u32x4 uP = {pack16<F16>(p0.x, p0.y), pack16<F16>(p0.z, p0.w), pack16<F16>(p1.x, p1.y), pack16<F16>(p1.z, p1.w)};
      const u32x4 uQ = {pack16<F16>(r0.x, r0.y), pack16<F16>(r0.z, r0.w), pack16<F16>(r1.x, r1.y), pack16<F16>(r1.z, r1.w)};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const u32x4 wf = *reinterpret_cast<const u32x4*>(wb + (size_t)s * d.w0_n * 32 + i * 512);
        st[2 * i] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, uP), st[2 * i]);
        st[2 * i + 1] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, uQ), st[2 * i + 1]);
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int cb = 3 * wave + (j >> 1), t = ((j & 1) ? fQ : fP) * 32 + lrow, gr = c0 + t;
      const bool inside = gr >= tile.seq_begin && gr < tile.seq_end;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int c = cb * 32 + 8 * rq + 4 * lk;
        const float4 b = *reinterpret_cast<const float4*>(d.b0 + c);
        const float v0 = (st[j][4 * rq] + b.x) + 0.0f, v1 = (st[j][4 * rq + 1] + b.y) + 0.0f;
        const float v2 = (st[j][4 * rq + 2] + b.z) + 0.0f, v3 = (st[j][4 * rq + 3] + b.w) + 0.0f;
        st[j][4 * rq] = v0; st[j][4 * rq + 1] = v1; st[j][4 * rq + 2] = v2; st[j][4 * rq + 3] = v3;
        *reinterpret_cast<uint2*>(xs + (t + 2) * WN_XP + c) = inside ? make_uint2(pack16<F16>(v0, v1), pack16<F16>(v2, v3)) : make_uint2(0u, 0u);
      }
    }
  } else {
    constexpr int Q4 = WN_XP / 4;  // 8-byte pieces of a window row
    for (int e = tid - 128; e < 4 * Q4; e += 128) {
      const int r = e / Q4, row = r < 2 ? r : WN_BM + r;  // 0, 1, 66, 67
      *reinterpret_cast<uint2*>(xs + row * WN_XP + (e % Q4) * 4) = make_uint2(0u, 0u);
    }
  }

  f32x16 acc[6], accc[6];
  auto xload = [&](bf16x8& xP, bf16x8& xQ, const unsigned short* xrow, int pitch) __attribute__((always_inline)) {
    xP = *reinterpret_cast<const bf16x8*>(xrow + (fP * 32 + lrow) * pitch + lk * 8);
    xQ = *reinterpret_cast<const bf16x8*>(xrow + (fQ * 32 + lrow) * pitch + lk * 8);
  };
  auto pair_step = [&](int slot, f32x16 (&a)[6], bf16x8& xP, bf16x8& xQ, const unsigned short* xnext, int pitch) __attribute__((always_inline)) {
    const bf16x8 cP = xP, cQ = xQ;
    xload(xP, xQ, xnext, pitch);
    arrive(slot);
    u32x4 wf[WN_L];
#pragma unroll
    for (int i = 0; i < WN_L; ++i) wf[i] = wr[slot][i];
    a[0] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[0]), cP, a[0]);
    a[1] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[0]), cQ, a[1]);
    a[2] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[1]), cP, a[2]);
    a[3] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[1]), cQ, a[3]);
    a[4] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[2]), cP, a[4]);
    a[5] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[3]), cP, a[5]);
    request(slot);
  };
  bf16x8 xP, xQ;
  auto window_at = [&](int s) __attribute__((always_inline)) {
    s = s < WN_STEPS1 ? s : WN_STEPS1 - 1;
    return xs + (s / (WN_H / 16)) * WN_XP + (s % (WN_H / 16)) * 16;
  };

#pragma unroll 1
  for (int i = 0; i < 4; ++i) {
    const float *b1 = pick(d.b1, i), *b2 = pick(d.b2, i);
    const void* w2 = pick(d.w2, i);
    const int n2 = i < 3 ? 2 * WN_H : WN_H, cbase = i < 3 ? 3 * wave : 3 * (wave & 1), ccol = i * 2 * WN_H;
    publish();  // (1) the window is complete (first layer: and g)
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    // ---- gated conv: tap-major, k ascending in 16-channel steps
    xload(xP, xQ, window_at(0), WN_XP);
#pragma unroll 1
    for (int base = 0; base < WN_STEPS1; base += WN_DEPTH) {
      if (base == WN_STEPS1 - WN_DEPTH) stream_pairs(d.wc, d.wc_n, ccol);
#pragma unroll
      for (int u = 0; u < WN_DEPTH; ++u) pair_step(u, acc, xP, xQ, window_at(base + u + 1), WN_XP);
    }
    // ---- cond = cond_conv(g)[this layer's 384 columns]
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) accc[j][r] = 0.0f;
    xload(xP, xQ, gs, WN_GP);
#pragma unroll 1
    for (int base = 0; base < WN_STEPSC; base += WN_DEPTH) {
      if (base == WN_STEPSC - WN_DEPTH) stream_res_skip(w2, n2, cbase);
#pragma unroll
      for (int u = 0; u < WN_DEPTH; ++u) {
        const int s1 = base + u + 1 < WN_STEPSC ? base + u + 1 : WN_STEPSC - 1;
        pair_step(u, accc, xP, xQ, gs + s1 * 16, WN_GP);
      }
    }
    // ---- acts = tanh(a + bias + cond) * sigmoid(g + bias + cond) -> LDS, 16-bit (the expressions of wavenet_layer_kernel)
    {
      auto gate = [&](const f32x16& aa, const f32x16& ag, const f32x16& ca, const f32x16& cg, int pb, int f) __attribute__((always_inline)) {
        const int t = f * 32 + lrow;
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int c = pb * 32 + 8 * rq + 4 * lk;
          const float4 ba = *reinterpret_cast<const float4*>(b1 + c), bg = *reinterpret_cast<const float4*>(b1 + WN_H + c);
          float pa[4], pg[4];
          const float4 ea = *reinterpret_cast<const float4*>(d.bc + ccol + c), eg = *reinterpret_cast<const float4*>(d.bc + ccol + WN_H + c);
          const float eav[4] = {ea.x, ea.y, ea.z, ea.w}, egv[4] = {eg.x, eg.y, eg.z, eg.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            pa[q] = (ca[4 * rq + q] + eav[q]) + 0.0f;
            pg[q] = (cg[4 * rq + q] + egv[q]) + 0.0f;
          }
          const float bav[4] = {ba.x, ba.y, ba.z, ba.w}, bgv[4] = {bg.x, bg.y, bg.z, bg.w};
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float av = aa[4 * rq + q] + bav[q] + pa[q], gvv = ag[4 * rq + q] + bgv[q] + pg[q];
            const float th = 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * av)) - 1.0f;
            v[q] = th * __builtin_amdgcn_rcpf(1.0f + __expf(-gvv));
          }
          *reinterpret_cast<uint2*>(as + t * WN_XP + c) = make_uint2(pack16<F16>(v[0], v[1]), pack16<F16>(v[2], v[3]));
        }
      };
      gate(acc[0], acc[2], accc[0], accc[2], P0, fP);
      gate(acc[1], acc[3], accc[1], accc[3], P0, fQ);
      gate(acc[4], acc[5], accc[4], accc[5], P1, fP);
#pragma unroll
      for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    }
    publish();  // (2) acts are complete (and every wave is done with the window)
    // ---- res / skip conv: acc[2 j] = block cbase + j over fP, acc[2 j + 1] over fQ
    xload(xP, xQ, as, WN_XP);
#pragma unroll 1
    for (int base = 0; base < WN_STEPS2; base += WN_DEPTH) {
      if (base == WN_STEPS2 - WN_DEPTH) {
        if (i < 3) {  // the requests of this block are the first k-steps of the next layer
          stream_pairs(pick(d.w1, i + 1), 2 * WN_H, 0);
        } else {  // nothing follows: the tail re-requests the last k-step (unused)
          q0 -= qs; q1 -= qs; q2 -= qs; q3 -= qs;
          qs = 0;
        }
      }
#pragma unroll
      for (int u = 0; u < WN_DEPTH; ++u) {
        const bf16x8 cP = xP, cQ = xQ;
        const int s1 = base + u + 1 < WN_STEPS2 ? base + u + 1 : WN_STEPS2 - 1;
        xload(xP, xQ, as + s1 * 16, WN_XP);
        arrive(u);
        u32x4 wf[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) wf[k] = wr[u][k];
        acc[0] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[0]), cP, acc[0]);
        acc[1] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[0]), cQ, acc[1]);
        acc[2] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[1]), cP, acc[2]);
        acc[3] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[1]), cQ, acc[3]);
        acc[4] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[2]), cP, acc[4]);
        acc[5] = mfma16<F16>(__builtin_bit_cast(bf16x8, wf[2]), cQ, acc[5]);
        request(u);
      }
    }
    // ---- state += res_skip + bias; waves 0, 1 write the next layer's window (zero outside the utterance)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int cb = cbase + (j >> 1), t = ((j & 1) ? fQ : fP) * 32 + lrow, gr = c0 + t;
      const bool inside = gr >= tile.seq_begin && gr < tile.seq_end;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int c = cb * 32 + 8 * rq + 4 * lk;
        const float4 b = *reinterpret_cast<const float4*>(b2 + c);
        const float v0 = (acc[j][4 * rq] + b.x) + st[j][4 * rq], v1 = (acc[j][4 * rq + 1] + b.y) + st[j][4 * rq + 1];
        const float v2 = (acc[j][4 * rq + 2] + b.z) + st[j][4 * rq + 2], v3 = (acc[j][4 * rq + 3] + b.w) + st[j][4 * rq + 3];
        st[j][4 * rq] = v0; st[j][4 * rq + 1] = v1; st[j][4 * rq + 2] = v2; st[j][4 * rq + 3] = v3;
        if (i < 3 && wave < 2)
          *reinterpret_cast<uint2*>(xs + (t + 2) * WN_XP + c) = inside ? make_uint2(pack16<F16>(v0, v1), pack16<F16>(v2, v3)) : make_uint2(0u, 0u);
      }
    }
  }
  TTS_WAIT_VM(0);  // drain the tail requests: their destination registers stay allocated (pinned) until here
#pragma unroll
  for (int u = 0; u < WN_DEPTH; ++u) {
    TTS_PIN(wr[u][0]);
    TTS_PIN(wr[u][1]);
    TTS_PIN(wr[u][2]);
    TTS_PIN(wr[u][3]);
  }
  // ---- the tail: [m | logs] = end(skip sum), the coupling, the inverse 1x1 conv and ActNorm; the new x is all that is written.
  // `end` in the arithmetic of the stand-alone launch (gemm_rows_kernel's fp32 branch in conv1d.hip): v_mfma_f32_32x32x2_f32 with
  // the weights as the first operand, one accumulator chain per output half, channel groups g ascending, MFMA j of a group
  // contracting channels 8 g + j and 8 g + 4 + j.  Wave cb = 0, 1, 2 owns output columns 32 cb .. 32 cb + 31 of both halves over
  // both frame blocks (of block 2 only columns 64 .. 79 are real; wave 3 has nothing to do), so every weight is fetched once per
  // workgroup and feeds two MFMAs, m and logs of an element meet in one lane, and a lane's four consecutive columns n .. n + 3 are
  // the x1 inputs of the two mixing groups n / 2 and n / 2 + 1, whose x0 inputs are columns n .. n + 3 of x: the mix needs no other
  // lane.  A row's values depend on that row of the skip sum alone, so the halo rows' results are simply not stored.
  // The weights are fp32 [192][we_n]: a lane's operand is one dword per (row, half), eight loads per group.  They run as a stream
  // like the layers' (inline-asm loads, counted waits), WE_DEPTH groups ahead: left to the compiler, the loads were scheduled next
  // to their uses and every group paid an L2 round trip (the launch took 141 us with them, 121 us with the stream; 104 us is the launch
  // without the tail).  The rows of x the epilogue needs are requested in front of the stream, so its first wait covers them.  The
  // requests follow the skip sum's way into LDS: issued in front of it, while the state registers are still live, the kernel spilled.
  constexpr int NF = 2, NG = WN_H / 8, WE_DEPTH = 4, WE_L = 8, XL = NF * 4 * 2;
  static_assert(NG % WE_DEPTH == 0 && XL + WE_DEPTH * WE_L < 64, "whole blocks of groups; the loads in flight fit the vmcnt counter");
  const int cb = wave;
  u32x4 x0u[NF][4], axu[NF][4];  // the rows of x the epilogue needs: requested in front of the stream, so its first wait covers them
  unsigned int wv[WE_DEPTH][2][4];
  const char* wq = reinterpret_cast<const char*>(d.we + (size_t)(4 * lk) * d.we_n + cb * 32 + lrow);  // rows 8 g + 4 lk + j, this lane's column
  const size_t wrow = (size_t)d.we_n * 4, whalf = (size_t)d.we_half * 4;
  size_t wstep = 8 * wrow;
  auto wrequest = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      TTS_GLOAD32(wv[slot][0][j], wq + j * wrow);
      TTS_GLOAD32(wv[slot][1][j], wq + j * wrow + whalf);
    }
    wq += wstep;
  };
  // the epilogue's per-channel operands [end bias m | logs][ActNorm bias][exp(-ActNorm logs)] go through LDS (behind the skip sum): read
  // from memory in the epilogue, each group of four columns paid a round trip behind the stores of the group before it
  // (staged by wave 3, which has no part in the product and no loads of the stream in flight)
  float* ep = sk + WN_BM * WB_SP;
  // The skip sum crosses LDS once, in fp32 (waves 2, 3 each hold half of its channels); every wave has passed the last layer's
  // barrier (2), so the window and g are free, and acts, which slower waves may still read, are not touched.
  if (wave >= 2) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int sb = 3 * (wave - 2) + (j >> 1), t = ((j & 1) ? fQ : fP) * 32 + lrow;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq)
        *reinterpret_cast<float4*>(sk + t * WB_SP + sb * 32 + 8 * rq + 4 * lk) = make_float4(st[j][4 * rq], st[j][4 * rq + 1], st[j][4 * rq + 2], st[j][4 * rq + 3]);
    }
  }
  if (wave < 3) {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const float* xr = d.x + (size_t)clamp_row(c0 + i * 32 + lrow) * d.ld_x;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        int n = cb * 32 + 8 * rq + 4 * lk;
        n = n < WB_COUT ? n : WB_COUT - 4;  // (block 2: the columns past 79 load real ones and are dropped)
        TTS_GLOAD128(x0u[i][rq], xr + n);
        TTS_GLOAD128(axu[i][rq], xr + WB_COUT + n);
      }
    }
#pragma unroll
    for (int u = 0; u < WE_DEPTH; ++u) wrequest(u);
  }
  if (wave == 3) {
#pragma unroll 1
    for (int e = lane; e < 3 * WB_X / 4; e += 64) {
      const int which = e / (WB_X / 4), c4 = 4 * (e % (WB_X / 4));
      float4 v = *reinterpret_cast<const float4*>((which == 0 ? d.be : (which == 1 ? d.an_bias : d.an_logs)) + c4);
      if (which == 2) v = make_float4(glow_actnorm_scale(v.x), glow_actnorm_scale(v.y), glow_actnorm_scale(v.z), glow_actnorm_scale(v.w));
      *reinterpret_cast<float4*>(ep + 4 * e) = v;
    }
  }
  publish();  // (3) the skip sum is complete
  if (wave < 3) {
    auto u2f = [](unsigned int bits) __attribute__((always_inline)) { return __builtin_bit_cast(float, bits); };
    f32x16 am[NF], al[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        am[i][r] = 0.0f;
        al[i][r] = 0.0f;
      }
    const float* skr = sk + lrow * WB_SP + 4 * lk;
#pragma unroll 1
    for (int base = 0; base < NG; base += WE_DEPTH) {
      if (base == NG - WE_DEPTH) {  // nothing follows: the tail re-requests the last group (unused), no branch in the stream
        wq -= wstep;
        wstep = 0;
      }
#pragma unroll
      for (int u = 0; u < WE_DEPTH; ++u) {
        float4 bq[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) bq[i] = *reinterpret_cast<const float4*>(skr + i * 32 * WB_SP + 8 * (base + u));
        TTS_WAIT_VM((WE_DEPTH - 1) * WE_L);
        float wm[4], wl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          TTS_PIN(wv[u][0][j]);
          TTS_PIN(wv[u][1][j]);
          wm[j] = u2f(wv[u][0][j]);  // copies: the slot is re-requested below while the MFMAs may still read
          wl[j] = u2f(wv[u][1][j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < NF; ++i) {
            const float bv = j == 0 ? bq[i].x : (j == 1 ? bq[i].y : (j == 2 ? bq[i].z : bq[i].w));
            am[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wm[j], bv, am[i], 0, 0, 0);
            al[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[j], bv, al[i], 0, 0, 0);
          }
        wrequest(u);
      }
    }
    TTS_WAIT_VM(0);  // drain the tail requests
#pragma unroll
    for (int u = 0; u < WE_DEPTH; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        TTS_PIN(wv[u][0][j]);
        TTS_PIN(wv[u][1][j]);
      }
    float4 x0v[NF][4], axv[NF][4];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        TTS_PIN(x0u[i][rq]);
        TTS_PIN(axu[i][rq]);
        const u32x4 p = x0u[i][rq], q = axu[i][rq];
        x0v[i][rq] = make_float4(u2f(p[0]), u2f(p[1]), u2f(p[2]), u2f(p[3]));
        axv[i][rq] = make_float4(u2f(q[0]), u2f(q[1]), u2f(q[2]), u2f(q[3]));
      }
    float w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = d.winv[i];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const int t = i * 32 + lrow, row = c0 + t;
      if (t < WB_HALO || t >= WB_HALO + WB_OUT || row >= tile.seq_end) continue;
      float* orow = d.x_out + (size_t)row * d.ld_out;
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int n = cb * 32 + 8 * rq + 4 * lk;
        if (n >= WB_COUT) continue;
        const float4 bm = *reinterpret_cast<const float4*>(ep + n), bl = *reinterpret_cast<const float4*>(ep + WB_COUT + n);
        const float bmv[4] = {bm.x, bm.y, bm.z, bm.w}, blv[4] = {bl.x, bl.y, bl.z, bl.w};
        const float axq[4] = {axv[i][rq].x, axv[i][rq].y, axv[i][rq].z, axv[i][rq].w};
        float y[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // epilogue_value<true> of the coupling conv (conv_epilogue.h): no per-utterance vector, no pre-add, no residual
          const float m = am[i][4 * rq + q] + bmv[q] + 0.0f, logs = al[i][4 * rq + q] + blv[q];
          y[q] = glow_coupling_value(axq[q], m, logs);
          y[q] *= d.alpha;
        }
        // mixing groups n / 2 and n / 2 + 1: slots (x0[n], x0[n + 1], x1[n], x1[n + 1]) and (x0[n + 2], x0[n + 3], x1[n + 2], x1[n + 3])
        const float4 b0 = *reinterpret_cast<const float4*>(ep + WB_X + n), b1 = *reinterpret_cast<const float4*>(ep + WB_X + WB_COUT + n);
        const float4 l0 = *reinterpret_cast<const float4*>(ep + 2 * WB_X + n), l1 = *reinterpret_cast<const float4*>(ep + 2 * WB_X + WB_COUT + n);
        const float4 xa = x0v[i][rq];
        *reinterpret_cast<float4*>(orow + n) = make_float4(glow_mix_value(w, 0, xa.x, xa.y, y[0], y[1], b0.x, l0.x), glow_mix_value(w, 1, xa.x, xa.y, y[0], y[1], b0.y, l0.y),
                                                           glow_mix_value(w, 0, xa.z, xa.w, y[2], y[3], b0.z, l0.z), glow_mix_value(w, 1, xa.z, xa.w, y[2], y[3], b0.w, l0.w));
        *reinterpret_cast<float4*>(orow + WB_COUT + n) = make_float4(glow_mix_value(w, 2, xa.x, xa.y, y[0], y[1], b1.x, l1.x), glow_mix_value(w, 3, xa.x, xa.y, y[0], y[1], b1.y, l1.y),
                                                                     glow_mix_value(w, 2, xa.z, xa.w, y[2], y[3], b1.z, l1.z), glow_mix_value(w, 3, xa.z, xa.w, y[2], y[3], b1.w, l1.w));
      }
    }
  }
}

namespace {
int wavenet_launch(const TtsWavenetDesc& d, const WavenetCond* c, hipStream_t st) {
  TTS_CHECK_ARG(d.hs_in && d.hs_out && d.w1 && d.b1 && d.w2 && d.b2 && d.tiles, "wavenet_layer: null pointer");
  TTS_CHECK_ARG(d.hs_in != d.hs_out, "wavenet_layer: the hidden state cannot be updated in place (the 5-tap conv reads neighbouring tiles)");
  TTS_CHECK_ARG(d.cout2 == 384 || d.cout2 == 192, "wavenet_layer: res/skip width %d (384, or 192 for the last layer)", d.cout2);
  TTS_CHECK_ARG(d.compute == TTS_COMPUTE_BF16 || d.compute == TTS_COMPUTE_F16, "wavenet_layer: 16-bit MFMA configurations only (compute %d)", d.compute);
  TTS_CHECK_ARG(d.tile_rows == WN_BM, "wavenet_layer: tile table must use %d rows, got %d", WN_BM, d.tile_rows);
  TTS_CHECK_ARG((d.ld_in & 3) == 0 && (d.ld_out & 3) == 0 && ((uintptr_t)d.hs_in & 15) == 0 && ((uintptr_t)d.hs_out & 15) == 0 && ((uintptr_t)d.w1 & 15) == 0 &&
                    ((uintptr_t)d.w2 & 15) == 0 && ((uintptr_t)d.b1 & 15) == 0 && ((uintptr_t)d.b2 & 15) == 0,
                "wavenet_layer: rows and weights must be 16-byte aligned");
  if (c) {
    TTS_CHECK_ARG(c->g && c->wc && c->bc, "wavenet_layer: null conditioning pointer");
    TTS_CHECK_ARG(c->ld_g >= WN_G && (c->ld_g & 3) == 0 && c->col0 >= 0 && (c->col0 & 31) == 0 && c->col0 + 2 * WN_H <= c->wc_n,
                  "wavenet_layer: conditioning columns %d .. of %d, row stride %d", c->col0, c->wc_n, c->ld_g);
    TTS_CHECK_ARG(((uintptr_t)c->g & 15) == 0 && ((uintptr_t)c->wc & 15) == 0 && ((uintptr_t)c->bc & 15) == 0, "wavenet_layer: conditioning operands must be 16-byte aligned");
  } else {
    TTS_CHECK_ARG(d.cond, "wavenet_layer: null pointer");
    TTS_CHECK_ARG((d.ld_cond & 3) == 0 && ((uintptr_t)d.cond & 15) == 0, "wavenet_layer: rows and weights must be 16-byte aligned");
  }
  if (d.n_tiles == 0) return TTS_OK;
  const bool f16 = d.compute == TTS_COMPUTE_F16;
  const WavenetCond none = {nullptr, 0, nullptr, 0, 0, nullptr};
  if (c) {
    const size_t lds = WN_XS_BYTES + WN_GS_BYTES;  // above the 64 KB a kernel gets without asking
    static unsigned long long raised[2] = {0, 0};
    const void* k = f16 ? reinterpret_cast<const void*>(wavenet_layer_kernel<true, true>) : reinterpret_cast<const void*>(wavenet_layer_kernel<false, true>);
    if (raise_lds_limit(k, raised[f16 ? 1 : 0]) != hipSuccess) {
      set_error("wavenet_layer: raising the dynamic LDS limit failed");
      return TTS_E_LAUNCH;
    }
    if (f16) hipLaunchKernelGGL((wavenet_layer_kernel<true, true>), dim3(d.n_tiles), dim3(256), lds, st, d, *c);
    else hipLaunchKernelGGL((wavenet_layer_kernel<false, true>), dim3(d.n_tiles), dim3(256), lds, st, d, *c);
  } else {
    if (f16) hipLaunchKernelGGL((wavenet_layer_kernel<true, false>), dim3(d.n_tiles), dim3(256), WN_XS_BYTES, st, d, none);
    else hipLaunchKernelGGL((wavenet_layer_kernel<false, false>), dim3(d.n_tiles), dim3(256), WN_XS_BYTES, st, d, none);
  }
  return launch_status("wavenet_layer");
}
}  // namespace

int wavenet_block_tile_rows() { return WB_OUT; }

int wavenet_block(const WavenetBlock& d, hipStream_t st) {
  TTS_CHECK_ARG(d.x && d.w0 && d.b0 && d.x_out && d.g && d.wc && d.bc && d.tiles, "wavenet_block: null pointer");
  TTS_CHECK_ARG(d.we && d.be && d.winv && d.an_bias && d.an_logs, "wavenet_block: null pointer (end conv, inverse 1x1 conv or ActNorm)");
  TTS_CHECK_ARG(d.x_out != d.x, "wavenet_block: x cannot be updated in place (a workgroup reads its neighbours' rows of x0, and the inverse 1x1 conv changes every channel)");
  TTS_CHECK_ARG(((uintptr_t)d.we & 15) == 0 && ((uintptr_t)d.be & 15) == 0 && ((uintptr_t)d.winv & 15) == 0 && ((uintptr_t)d.an_bias & 15) == 0 &&
                    ((uintptr_t)d.an_logs & 15) == 0 && ((uintptr_t)d.x_out & 15) == 0,
                "wavenet_block: x_out, the end conv, the inverse 1x1 conv and ActNorm must be 16-byte aligned");
  TTS_CHECK_ARG(d.we_half >= 96 && d.we_n >= d.we_half + 96, "wavenet_block: the end conv has %d packed columns (logs from %d): three blocks of 32 per half are read", d.we_n, d.we_half);
  TTS_CHECK_ARG(d.n_pad >= 0 && (d.n_pad == 0 || d.pad_rows), "wavenet_block: %d rows outside the tiles, no row table", d.n_pad);
  for (int i = 0; i < 4; ++i) {
    TTS_CHECK_ARG(d.w1[i] && d.b1[i] && d.w2[i] && d.b2[i], "wavenet_block: null weights of layer %d", i);
    TTS_CHECK_ARG(((uintptr_t)d.w1[i] & 15) == 0 && ((uintptr_t)d.w2[i] & 15) == 0 && ((uintptr_t)d.b1[i] & 15) == 0 && ((uintptr_t)d.b2[i] & 15) == 0,
                  "wavenet_block: weights must be 16-byte aligned");
  }
  TTS_CHECK_ARG(d.compute == TTS_COMPUTE_BF16 || d.compute == TTS_COMPUTE_F16, "wavenet_block: 16-bit MFMA configurations only (compute %d)", d.compute);
  TTS_CHECK_ARG(d.tile_rows == WB_OUT, "wavenet_block: tile table must use %d rows, got %d", WB_OUT, d.tile_rows);
  TTS_CHECK_ARG(d.ld_x >= WB_X && (d.ld_x & 3) == 0 && d.ld_out >= WB_X && (d.ld_out & 3) == 0 && d.ld_g >= WN_G && (d.ld_g & 3) == 0 &&
                    ((uintptr_t)d.x & 15) == 0 && ((uintptr_t)d.g & 15) == 0 && ((uintptr_t)d.wc & 15) == 0 && ((uintptr_t)d.bc & 15) == 0 &&
                    ((uintptr_t)d.w0 & 15) == 0 && ((uintptr_t)d.b0 & 15) == 0,
                "wavenet_block: rows, start and conditioning operands must be 16-byte aligned");
  TTS_CHECK_ARG(d.w0_n >= WN_H, "wavenet_block: the start conv has %d packed columns, the hidden state %d", d.w0_n, WN_H);
  TTS_CHECK_ARG(d.wc_n >= 8 * WN_H, "wavenet_block: %d conditioning columns, four layers need %d", d.wc_n, 8 * WN_H);
  const int pad_blocks = (d.n_pad * WB_MIXG + 255) / 256;  // workgroups behind the tile table, for the rows outside the tiles
  if (d.n_tiles + pad_blocks == 0) return TTS_OK;
  const bool f16 = d.compute == TTS_COMPUTE_F16;
  static unsigned long long raised[2] = {0, 0};
  const void* k = f16 ? reinterpret_cast<const void*>(wavenet_block_kernel<true>) : reinterpret_cast<const void*>(wavenet_block_kernel<false>);
  if (raise_lds_limit(k, raised[f16 ? 1 : 0]) != hipSuccess) {
    set_error("wavenet_block: raising the dynamic LDS limit failed");
    return TTS_E_LAUNCH;
  }
  if (f16) hipLaunchKernelGGL((wavenet_block_kernel<true>), dim3(d.n_tiles + pad_blocks), dim3(256), WB_LDS_BYTES, st, d);
  else hipLaunchKernelGGL((wavenet_block_kernel<false>), dim3(d.n_tiles + pad_blocks), dim3(256), WB_LDS_BYTES, st, d);
  return launch_status("wavenet_block");
}

int wavenet_layer(const TtsWavenetDesc& d, hipStream_t st) { return wavenet_launch(d, nullptr, st); }

int wavenet_layer_cond(const TtsWavenetDesc& d, const WavenetCond& c, hipStream_t st) { return wavenet_launch(d, &c, st); }

}  // namespace tts

extern "C" int tts_wavenet_layer(const TtsWavenetDesc* d, tts_stream_t stream) {
  if (!d) {
    tts::set_error("tts_wavenet_layer: null descriptor");
    return TTS_E_ARG;
  }
  return tts::wavenet_layer(*d, reinterpret_cast<hipStream_t>(stream));
}
