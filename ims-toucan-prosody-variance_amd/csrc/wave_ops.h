// The cross-lane reductions and scans of the analysis kernels, each order spelled once ("Summation orders").  A
// floating-point result depends on the order of its additions, and "alone == in a batch, bit for bit" holds because every kernel
// takes its order from here:
//   butterfly + left fold   wave_fold / block_fold and what is named after them (wave_sum, block_sum, wave_max, block_max)
//   256-entry LDS tree      block_tree_fold: a DIFFERENT order, not interchangeable with the butterfly without changing results
//   in-order walk           wave_each_in_order: the plain sequential order, every lane doing all of it
// The arg-best butterfly and the scans are exact (comparisons and integers), so their order shows only in the tie rule.
// Device code only.  A wavefront has 64 lanes; a workgroup is WAVES wavefronts and its thread index is threadIdx.x.
#pragma once
#include "common.h"

namespace tts {

// ---- wavefront layer: no LDS, no barrier -----------------------------------------------------------------------------------------
// The xor butterfly WIDTH/2 .. 1 over an associative op: every lane of a group of WIDTH gets op over the group.  At each step a
// lane computes op(its own, its partner's); the whole wavefront must be converged.
template <int WIDTH = 64, class T, class Op>
__device__ __forceinline__ T wave_fold(T v, Op op) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, WIDTH));
  return v;
}

__device__ __forceinline__ float wave_sum(float v) {
  return wave_fold(v, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ double wave_sum(double v) {
  return wave_fold(v, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ long long wave_sum(long long v) {
  return wave_fold(v, [](long long a, long long b) { return a + b; });
}
__device__ __forceinline__ float wave_max(float v) {
  return wave_fold(v, [](float a, float b) { return fmaxf(a, b); });
}

// ---- workgroup layer -------------------------------------------------------------------------------------------------------------
// The slots of the wavefronts folded left to right: ((r0 op r1) op r2) op r3.
template <int WAVES = 4, class T, class Op>
__device__ __forceinline__ T fold_left(const T* red, Op op) {
  T r = red[0];
#pragma unroll
  for (int k = 1; k < WAVES; ++k) r = op(r, red[k]);
  return r;
}

// op over the workgroup: the butterfly, lane 0 of each wavefront writes its slot of red[WAVES] (LDS), the slots are folded left
// to right.  Contract: every thread of the workgroup calls it; it has two barriers, one before red is written (the call before
// may still be reading it) and one after, so calls back to back on the same red are safe; all threads get the result.
template <int WAVES = 4, class T, class Op>
__device__ __forceinline__ T block_fold(T v, T* red, Op op) {
  v = wave_fold(v, op);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fold_left<WAVES>(red, op);
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  return block_fold(v, red, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ double block_sum(double v, double* red) {
  return block_fold(v, red, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ long long block_sum(long long v, long long* red) {
  return block_fold(v, red, [](long long a, long long b) { return a + b; });
}
__device__ __forceinline__ float block_max(float v, float* red) {
  return block_fold(v, red, [](float a, float b) { return fmaxf(a, b); });
}

// ---- first best of (value, index) ------------------------------------------------------------------------------------------------
// The one tie rule: (ov, oi) goes before (v, i) if ov is better, or equal and oi < i.  MAX: better is greater; else smaller.
template <bool MAX, class T>
__device__ __forceinline__ bool arg_before(T ov, int oi, T v, int i) {
  return (MAX ? ov > v : ov < v) || (ov == v && oi < i);
}

// (v, i) <- the best pair of the group of WIDTH lanes, in every lane of it.
template <int WIDTH, bool MAX, class T>
__device__ __forceinline__ void wave_arg_best(T& v, int& i) {
#pragma unroll
  for (int o = WIDTH / 2; o > 0; o >>= 1) {
    const T ov = __shfl_xor(v, o, WIDTH);
    const int oi = __shfl_xor(i, o, WIDTH);
    if (arg_before<MAX>(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
}
template <int WIDTH = 64, class T>
__device__ __forceinline__ void wave_arg_max(T& v, int& i) { wave_arg_best<WIDTH, true>(v, i); }
template <int WIDTH = 64, class T>
__device__ __forceinline__ void wave_arg_min(T& v, int& i) { wave_arg_best<WIDTH, false>(v, i); }

// ---- inclusive scans in thread order ---------------------------------------------------------------------------------------------
// forward: lane l gets op over lanes 0 .. l;  backward: over lanes l .. 63.
template <class T, class Op>
__device__ __forceinline__ T wave_scan_forward(T v, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T n = __shfl_up(v, o, 64);
    if (lane >= o) v = op(v, n);
  }
  return v;
}
template <class T, class Op>
__device__ __forceinline__ T wave_scan_backward(T v, Op op) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T n = __shfl_down(v, o, 64);
    if (lane + o < 64) v = op(v, n);
  }
  return v;
}

// The workgroup forms: thread t gets op over threads 0 .. t (forward) or t .. 64 WAVES - 1 (backward), *all = op over all.  The
// wavefront scan, its last (first) lane to red[WAVES], then the carry-in of the lower (higher) wavefronts.  The contract is
// block_fold's: every thread calls, two barriers, back-to-back calls on the same red are safe.
template <int WAVES = 4, class T, class Op>
__device__ __forceinline__ T block_scan_forward(T v, T* red, T* all, Op op) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_scan_forward(v, op);
  __syncthreads();
  if (lane == 63) red[wv] = v;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < WAVES; ++k)
    if (k < wv) v = op(v, red[k]);
  *all = fold_left<WAVES>(red, op);
  return v;
}
template <int WAVES = 4, class T, class Op>
__device__ __forceinline__ T block_scan_backward(T v, T* red, T* all, Op op) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_scan_backward(v, op);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < WAVES; ++k)
    if (k > wv) v = op(v, red[k]);
  *all = fold_left<WAVES>(red, op);
  return v;
}

// ---- the in-order walk -----------------------------------------------------------------------------------------------------------
// f(i, lane i's v ...) for i = 0 .. steps - 1 in turn, in every lane alike: the plain sequential order over the values the lanes
// hold, at the price of every lane doing all of it.  steps <= 64 is uniform; the whole wavefront calls it.
template <class F, class... T>
__device__ __forceinline__ void wave_each_in_order(int steps, F f, T... v) {
  for (int i = 0; i < steps; ++i) f(i, __shfl(v, i, 64)...);
}

// ---- the 256-entry LDS tree ------------------------------------------------------------------------------------------------------
// op over a workgroup of exactly 256 threads by halving red256[256]: 128 pairs (t, t + 128), then 64, ... 1.  NOT the butterfly's
// order: element t meets t + 128 first here, t ^ 32 within its wavefront there, so a floating-point sum moved from one to the other
// changes in its last bits.  Every thread calls it; it ends with a barrier, so red256 may be reused at once; all get the result.
template <class T, class Op>
__device__ __forceinline__ T block_tree_fold(T v, T* red256, Op op) {
  const int tid = threadIdx.x;
  red256[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red256[tid] = op(red256[tid], red256[tid + o]);
    __syncthreads();
  }
  const T r = red256[0];
  __syncthreads();
  return r;
}

}  // namespace tts
