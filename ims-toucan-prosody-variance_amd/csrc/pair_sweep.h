// The banded anti-diagonal sweep of a two-sequence dynamic programme with back-pointers, one workgroup of 256 per pair: what the
// time warping (compare.hip) and the edit distance (pronunciation.hip) share.  A kernel adds its cells (a policy, below) and its
// walk back along the pointers.
//
// The rows are taken in bands of 256: in a band thread t owns row i = band + t and keeps what belongs to the row in registers; at
// step s of the band's anti-diagonal sweep it forms the cell (i, s - t), so the other sequence streams.  D of the last two
// anti-diagonals lies in LDS (diag[2][256]): D(i-1, j) is what thread t - 1 wrote a step ago, D(i-1, j-1) is what this thread read
// there a step ago and kept, D(i, j-1) is its own last value.  Thread 0 takes both from row[], D of the band before's last row (or
// the policy's border), which thread 255 overwrites 255 columns behind thread 0's reads.  One barrier per step.  The predecessor
// is the diagonal one, then the upper one if strictly smaller, then the left one if strictly smaller (codes 0, 1, 2).
// Back-pointers: 2 bits per cell in rows of whole words, a thread collecting 16 of its row in a register before it stores the
// word - to LDS (a negative scratch offset) or to the caller's scratch; a fence and a barrier close the sweep, after which any
// thread may read them (bp_code).
//
// A policy P supplies
//   value_t, ORIGIN                the type of D; the index of the first row and column (rows i = ORIGIN .. ORIGIN + rows - 1)
//   band(i, active)                the row's own registers, at the head of every band
//   border(i, j)                   D(i, j) where i or j is ORIGIN - 1
//   step(j, active)                every step, whether or not the thread has a cell
//   via(code, pred, j)             the candidate that predecessor `pred` makes when reached by `code`: what is compared
//   cell(i, j, best)               D(i, j) from the chosen candidate
//   last(D)                        at the last cell
#pragma once
#include "common.h"

namespace tts {

constexpr int SWEEP_THREADS = 256;

__host__ __device__ inline long long bp_words(int rows, int cols) { return (long long)rows * ((cols + 15) >> 4); }

// host code, beside bp_words which sizes what it checks: pair p's back-pointers fit the LDS asked for (a negative offset) or lie
// inside the scratch buffer
inline int check_bp_slot(const char* what, int p, long long bytes, long long off, int lds_bp_bytes, long long scratch_bytes) {
  if (off < 0)
    TTS_CHECK_ARG(bytes <= lds_bp_bytes, "%s: pair %d: %lld bytes of back-pointers do not fit the %d bytes of LDS asked for", what, p, bytes,
                  lds_bp_bytes);
  else
    TTS_CHECK_ARG(off % 4 == 0 && off + bytes <= scratch_bytes,
                  "%s: pair %d: %lld bytes of back-pointers at %lld do not fit the scratch buffer (%lld bytes)", what, p, bytes, off, scratch_bytes);
  return TTS_OK;
}

// the code of cell (i, j), both counted from ORIGIN; W = (cols + 15) >> 4
template <int ORIGIN = 0>
__device__ __forceinline__ unsigned int bp_code(const unsigned int* bp, int W, int i, int j) {
  return (bp[(size_t)(i - ORIGIN) * W + ((j - ORIGIN) >> 4)] >> (2 * ((j - ORIGIN) & 15))) & 3u;
}

// row: cols values from ORIGIN on; diag: 2 * 256 values.  The whole workgroup calls it -> the back-pointers.
template <class P>
__device__ __forceinline__ unsigned int* pair_sweep(P& pol, int rows, int cols, typename P::value_t* row, typename P::value_t* diag,
                                                    long long scratch_off, unsigned char* lds_bp, unsigned char* scratch) {
  using V = typename P::value_t;
  constexpr int O = P::ORIGIN;
  const int tid = threadIdx.x, W = (cols + 15) >> 4;
  const bool in_lds = scratch_off < 0;
  unsigned int* bp = in_lds ? reinterpret_cast<unsigned int*>(lds_bp) : reinterpret_cast<unsigned int*>(scratch + scratch_off);
  for (int i0 = 0; cols > 0 && i0 < rows; i0 += SWEEP_THREADS) {
    const int i = i0 + tid + O;
    const bool active = i < rows + O;
    const bool feeds_next = tid == SWEEP_THREADS - 1 && i0 + SWEEP_THREADS < rows;  // this row is the next band's row[]
    const int steps = min(SWEEP_THREADS, rows - i0) + cols - 1;
    pol.band(i, active);
    V left = pol.border(i, O - 1), kept_up = pol.border(i - 1, O - 1);
    unsigned int word = 0;
    unsigned int* bp_row = bp + (size_t)(i - O) * W;
    for (int s = 0; s < steps; ++s) {
      const int j = s - tid + O;
      const bool cell = active && j >= O && j < cols + O;
      pol.step(j, active);
      if (cell) {
        const V up = tid == 0 ? (i0 == 0 ? pol.border(O - 1, j) : row[j]) : diag[((s - 1) & 1) * SWEEP_THREADS + tid - 1];
        V best = pol.via(0, kept_up, j);
        unsigned int code = 0;
        const V c1 = pol.via(1, up, j);
        if (c1 < best) {
          best = c1;
          code = 1;
        }
        const V c2 = pol.via(2, left, j);
        if (c2 < best) {
          best = c2;
          code = 2;
        }
        const V D = pol.cell(i, j, best);
        kept_up = up;
        left = D;
        diag[(s & 1) * SWEEP_THREADS + tid] = D;
        if (feeds_next) row[j] = D;
        const int jj = j - O;
        word |= code << (2 * (jj & 15));
        if ((jj & 15) == 15 || j == cols - 1 + O) {
          bp_row[jj >> 4] = word;
          word = 0;
        }
        if (i == rows - 1 + O && j == cols - 1 + O) pol.last(D);
      }
      __syncthreads();
    }
  }
  if (!in_lds) __threadfence_block();
  __syncthreads();
  return bp;
}

}  // namespace tts
