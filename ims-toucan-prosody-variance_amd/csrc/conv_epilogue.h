// The fused conv epilogue shared by every tile form of tts_conv1d (conv1d.hip, conv1d_wide.hip): one arithmetic per output element
// (epilogue_value), so all forms round alike, and the vector epilogue of the transposed 32 x 32 accumulator layout.
#pragma once
#include "common.h"

namespace tts {

// One output element of the fused epilogue, up to the store: a / g are the raw accumulators (g: the gate half in the dual modes),
// ba / bg the biases, sv the per-utterance vector, pa / pg the pre-add, ax the coupling input, rv the residual.  Shared by every
// accumulator layout, so all of them round alike.
template <bool DUAL>
__device__ __forceinline__ float epilogue_value(const TtsConvDesc& d, float a, float g, float ba, float bg, float sv, float pa, float pg, float ax,
                                                float rv) {
  float v = a + ba + sv;
  if (d.preadd) v += pa;
  if (DUAL) {
    g += bg;
    if (d.preadd) g += pg;
    if (d.mode == TTS_MODE_GLU) {
      v = v * (1.0f / (1.0f + expf(-g)));
    } else if (d.mode == TTS_MODE_GATED) {
      v = tanhf(v) * (1.0f / (1.0f + expf(-g)));
    } else {  // COUPLING
      v = glow_coupling_value(ax, v, g);
    }
  } else {
    if (d.act == TTS_ACT_RELU) v = fmaxf(v, 0.0f);
    else if (d.act == TTS_ACT_TANH) v = tanhf(v);
  }
  v *= d.alpha;
  if (d.res) v += d.res_scale * rv;
  return v;
}

// ... one element at a time (the layouts whose lanes hold single columns, and the ragged right edge of the others)
template <bool DUAL>
__device__ __forceinline__ void epilogue_element(const TtsConvDesc& d, int row, int n, float a, float g, float ba, float bg, float sv, bool io_f16) {
  const float pa = d.preadd ? d.preadd[(size_t)row * d.ld_preadd + n] : 0.0f;
  const float pg = (DUAL && d.preadd) ? d.preadd[(size_t)row * d.ld_preadd + d.cout + n] : 0.0f;
  const float ax = (DUAL && d.mode == TTS_MODE_COUPLING) ? d.aux[(size_t)row * d.ld_aux + n] : 0.0f;
  float rv = 0.0f;
  if (d.res)
    rv = (d.io_flags & TTS_IO_RES_BF16) ? load16(reinterpret_cast<const unsigned short*>(d.res)[(size_t)row * d.ld_res + n], io_f16)
                                        : d.res[(size_t)row * d.ld_res + n];
  float v = epilogue_value<DUAL>(d, a, g, ba, bg, sv, pa, pg, ax, rv);
  if (d.io_flags & TTS_IO_Y_BF16) {
    unsigned short* yp = reinterpret_cast<unsigned short*>(d.y) + (size_t)row * d.ldy + n;
    if (d.accumulate) v += load16(*yp, io_f16);
    *yp = store16(v, io_f16);
  } else {
    float* yp = d.y + (size_t)row * d.ldy + n;
    if (d.accumulate) v += *yp;
    *yp = v;
  }
}

// Can the epilogue move four consecutive columns of a row at a time?  (every tensor it touches: 16-byte (fp32) / 8-byte (16-bit)
// aligned base, leading dimension and half offset a multiple of four)
__device__ __forceinline__ bool epilogue_vec_ok(const TtsConvDesc& d) {
  auto al = [](const void* p, unsigned m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) == 0; };
  bool ok = (d.cout & 3) == 0 && (d.ldy & 3) == 0 && al(d.y, (d.io_flags & TTS_IO_Y_BF16) ? 8 : 16);
  if (d.bias) ok = ok && al(d.bias, 16);
  if (d.seqvec) ok = ok && (d.ld_seqvec & 3) == 0 && al(d.seqvec, 16);
  if (d.preadd) ok = ok && (d.ld_preadd & 3) == 0 && al(d.preadd, 16);
  if (d.res) ok = ok && (d.ld_res & 3) == 0 && al(d.res, (d.io_flags & TTS_IO_RES_BF16) ? 8 : 16);
  if (d.mode == TTS_MODE_COUPLING) ok = ok && (d.ld_aux & 3) == 0 && al(d.aux, 16);
  return ok;
}

// Epilogue of a TRANSPOSED 32x32 accumulator (weights were the MFMA A operand): row of the tile = lane&31, column =
// (reg&3) + 8*(reg>>2) + 4*(lane>>5) - a lane owns four groups of four consecutive output channels of ONE row, so bias, pre-add,
// residual, accumulate and the store move 8 (16-bit tensors) or 16 (fp32) bytes at a time.  (With the output channel on the lane -
// the untransposed layout - a 128 x 128 tile left through 64 two-byte stores per lane: 58 us of a 147 us launch at 256 -> 256
// channels x 3 taps, 122 of 211 us with a residual read the same way, 340 of 609 us in the 128 -> 256 up-sampler; measured with
// a diagnostic build that skipped the epilogue)  A row's pieces are written by one wavefront within a few
// hundred cycles: L2 merges them into whole lines.
// FAST_ONLY: the caller guarantees the common case below (epilogue_vec_ok, no pre-add, `eb` given - the wide tile's dispatch checks
// it on the host), so the element-wise paths are not compiled in (with 4 x 2 accumulators their run-time indexed tail loops put the
// accumulators into scratch memory).
template <int TM, int TN, int NH, bool DUAL, bool FAST_ONLY = false>
__device__ __forceinline__ void conv_epilogue_t(const TtsConvDesc& d, const TtsTile& tile, int n0, int wm, int wn, int lrow, int lk,
                                                const f32x16 (&acc)[NH][TM][TN], const float* eb = nullptr, int eb_n = 0) {
  const bool io_f16 = d.io_flags & TTS_IO_F16;  // format of the 16-bit tensors of this call (else bf16)
  const bool vec = epilogue_vec_ok(d);
  const bool y16 = d.io_flags & TTS_IO_Y_BF16, r16 = d.io_flags & TTS_IO_RES_BF16;
  if constexpr (!DUAL) {
    if (FAST_ONLY || (vec && !d.preadd && eb)) {
      // The common case (plain convs: bias, per-utterance vector, residual, accumulate).  What was measured on the 128 x 128 tile at
      // 256 -> 256 channels (clock stamps of a diagnostic build): main loop 41.7 k cycles, epilogue 21.9 k - not the stores (they drain in
      // 0.4 k), but sixteen dependent global-load round trips per lane (bias, vector, residual of each 4-channel group, each ~1.4 k
      // cycles, and behind earlier stores: loads and stores share the in-order vmcnt counter, so a load issued after a store is usable
      // only once that store is acknowledged).  Hence: bias and per-utterance vector come from LDS (`eb`, staged at kernel start), and
      // all residual / accumulate reads of a 32-row block are issued together, in front of its stores: one round trip per block.
      auto col_of = [&](int j, int rq) { return n0 + (wn * TN + j) * 32 + 8 * rq + 4 * lk; };
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = tile.row0 + (wm * TM + i) * 32 + lrow;
        const int rowc = row < tile.seq_end ? row : tile.seq_end - 1;  // (clamped: unconditional loads; rows behind the utterance are never stored)
        constexpr int NG = TN * 4, CH = 8;  // 4-channel groups of the block, and how many of them travel together (registers: 8 per group)
#pragma unroll
        for (int g0 = 0; g0 < NG; g0 += CH) {
        uint4 rv[CH], yv[CH];
#pragma unroll
          for (int g = 0; g < CH; ++g) {
            if (g0 + g >= NG) continue;
            const int j = (g0 + g) >> 2, rq = (g0 + g) & 3;
            int n = col_of(j, rq);
            n = n < d.cout ? n : d.cout - 4;
            rv[g] = make_uint4(0, 0, 0, 0);
            yv[g] = make_uint4(0, 0, 0, 0);
            if (d.res) {
              if (r16) {
                const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(d.res) + (size_t)rowc * d.ld_res + n);
                rv[g].x = u.x; rv[g].y = u.y;
              } else {
                rv[g] = *reinterpret_cast<const uint4*>(d.res + (size_t)rowc * d.ld_res + n);
              }
            }
            if (d.accumulate) {
              if (y16) {
                const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(d.y) + (size_t)rowc * d.ldy + n);
                yv[g].x = u.x; yv[g].y = u.y;
              } else {
                yv[g] = *reinterpret_cast<const uint4*>(d.y + (size_t)rowc * d.ldy + n);
              }
            }
          }
        __builtin_amdgcn_sched_barrier(0);  // (all loads of the chunk in front of its first store)
        if (row < tile.seq_end) {
#pragma unroll
          for (int g = 0; g < CH; ++g) {
            if (g0 + g >= NG) continue;
            const int j = (g0 + g) >> 2, rq = (g0 + g) & 3;
            const int n = col_of(j, rq);
            if (n >= d.cout) continue;
            const float4 ba = *reinterpret_cast<const float4*>(eb + (n - n0));
            const float4 sv = *reinterpret_cast<const float4*>(eb + eb_n + (n - n0));
            const uint4 ru = rv[g], yu = yv[g];
            float4 r4, y4;
            if (r16) r4 = make_float4(load16(ru.x & 0xFFFF, io_f16), load16(ru.x >> 16, io_f16), load16(ru.y & 0xFFFF, io_f16), load16(ru.y >> 16, io_f16));
            else r4 = make_float4(__builtin_bit_cast(float, ru.x), __builtin_bit_cast(float, ru.y), __builtin_bit_cast(float, ru.z), __builtin_bit_cast(float, ru.w));
            if (y16) y4 = make_float4(load16(yu.x & 0xFFFF, io_f16), load16(yu.x >> 16, io_f16), load16(yu.y & 0xFFFF, io_f16), load16(yu.y >> 16, io_f16));
            else y4 = make_float4(__builtin_bit_cast(float, yu.x), __builtin_bit_cast(float, yu.y), __builtin_bit_cast(float, yu.z), __builtin_bit_cast(float, yu.w));
            float v0 = epilogue_value<false>(d, acc[0][i][j][4 * rq + 0], 0.f, ba.x, 0.f, sv.x, 0.f, 0.f, 0.f, r4.x);
            float v1 = epilogue_value<false>(d, acc[0][i][j][4 * rq + 1], 0.f, ba.y, 0.f, sv.y, 0.f, 0.f, 0.f, r4.y);
            float v2 = epilogue_value<false>(d, acc[0][i][j][4 * rq + 2], 0.f, ba.z, 0.f, sv.z, 0.f, 0.f, 0.f, r4.z);
            float v3 = epilogue_value<false>(d, acc[0][i][j][4 * rq + 3], 0.f, ba.w, 0.f, sv.w, 0.f, 0.f, 0.f, r4.w);
            if (d.accumulate) { v0 += y4.x; v1 += y4.y; v2 += y4.z; v3 += y4.w; }
            if (y16) {
              uint2* yp = reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(d.y) + (size_t)row * d.ldy + n);
              *yp = make_uint2((unsigned int)store16(v0, io_f16) | ((unsigned int)store16(v1, io_f16) << 16),
                               (unsigned int)store16(v2, io_f16) | ((unsigned int)store16(v3, io_f16) << 16));
            } else {
              *reinterpret_cast<float4*>(d.y + (size_t)row * d.ldy + n) = make_float4(v0, v1, v2, v3);
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        }
      }
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = tile.row0 + (wm * TM + i) * 32 + lrow;
    if (row >= tile.seq_end) continue;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int n = n0 + (wn * TN + j) * 32 + 8 * rq + 4 * lk;
        if (n >= d.cout) continue;
        if (!vec) {
          for (int q = 0; q < 4 && n + q < d.cout; ++q) {
            const float ba = d.bias ? d.bias[n + q] : 0.0f;
            const float bg = (DUAL && d.bias) ? d.bias[d.cout + n + q] : 0.0f;
            const float sv = d.seqvec ? d.seqvec[(size_t)tile.seq_id * d.ld_seqvec + n + q] : 0.0f;
            epilogue_element<DUAL>(d, row, n + q, acc[0][i][j][4 * rq + q], acc[NH - 1][i][j][4 * rq + q], ba, bg, sv, io_f16);
          }
          continue;
        }
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        auto ld4 = [](const float* p) { return *reinterpret_cast<const float4*>(p); };
        const float4 ba = d.bias ? ld4(d.bias + n) : z4;
        const float4 bg = (DUAL && d.bias) ? ld4(d.bias + d.cout + n) : z4;
        const float4 sv = d.seqvec ? ld4(d.seqvec + (size_t)tile.seq_id * d.ld_seqvec + n) : z4;
        const float4 pa = d.preadd ? ld4(d.preadd + (size_t)row * d.ld_preadd + n) : z4;
        const float4 pg = (DUAL && d.preadd) ? ld4(d.preadd + (size_t)row * d.ld_preadd + d.cout + n) : z4;
        const float4 ax = (DUAL && d.mode == TTS_MODE_COUPLING) ? ld4(d.aux + (size_t)row * d.ld_aux + n) : z4;
        float4 rv = z4;
        if (d.res) {
          if (r16) {
            const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(d.res) + (size_t)row * d.ld_res + n);
            rv = make_float4(load16(u.x & 0xFFFF, io_f16), load16(u.x >> 16, io_f16), load16(u.y & 0xFFFF, io_f16), load16(u.y >> 16, io_f16));
          } else {
            rv = ld4(d.res + (size_t)row * d.ld_res + n);
          }
        }
        float v[4];
        v[0] = epilogue_value<DUAL>(d, acc[0][i][j][4 * rq + 0], acc[NH - 1][i][j][4 * rq + 0], ba.x, bg.x, sv.x, pa.x, pg.x, ax.x, rv.x);
        v[1] = epilogue_value<DUAL>(d, acc[0][i][j][4 * rq + 1], acc[NH - 1][i][j][4 * rq + 1], ba.y, bg.y, sv.y, pa.y, pg.y, ax.y, rv.y);
        v[2] = epilogue_value<DUAL>(d, acc[0][i][j][4 * rq + 2], acc[NH - 1][i][j][4 * rq + 2], ba.z, bg.z, sv.z, pa.z, pg.z, ax.z, rv.z);
        v[3] = epilogue_value<DUAL>(d, acc[0][i][j][4 * rq + 3], acc[NH - 1][i][j][4 * rq + 3], ba.w, bg.w, sv.w, pa.w, pg.w, ax.w, rv.w);
        if (y16) {
          uint2* yp = reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(d.y) + (size_t)row * d.ldy + n);
          if (d.accumulate) {
            const uint2 u = *yp;
            v[0] += load16(u.x & 0xFFFF, io_f16); v[1] += load16(u.x >> 16, io_f16);
            v[2] += load16(u.y & 0xFFFF, io_f16); v[3] += load16(u.y >> 16, io_f16);
          }
          *yp = make_uint2((unsigned int)store16(v[0], io_f16) | ((unsigned int)store16(v[1], io_f16) << 16),
                           (unsigned int)store16(v[2], io_f16) | ((unsigned int)store16(v[3], io_f16) << 16));
        } else {
          float4* yp = reinterpret_cast<float4*>(d.y + (size_t)row * d.ldy + n);
          if (d.accumulate) {
            const float4 u = *yp;
            v[0] += u.x; v[1] += u.y; v[2] += u.z; v[3] += u.w;
          }
          *yp = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
  }
}

}  // namespace tts
