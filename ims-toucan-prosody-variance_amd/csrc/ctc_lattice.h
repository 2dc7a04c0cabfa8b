// The CTC lattice of one utterance, a workgroup of 256: what the loss (score.hip) and its gradient (train.hip) share.  A kernel adds
// where the log-probabilities are staged, what it keeps of alpha, and its own last expression.
//
// The n targets become S = 2n + 1 extended states: blank, l1, blank, l2, ..., blank; lab[s] holds the state's symbol and, in bit
// 31, whether the skip s-2 -> s is allowed (into a label that differs from the label two states back).  The log-probabilities
// are the reference's fp32 log_softmax, (x - max) - log(sum exp(x - max)), one wavefront per frame; the forward variables are
// fp64, alpha_0 starting in the first blank or the first label, alpha_t(s) = lse3 of the up to three predecessors + lp_t(s); the
// log-likelihood ends in the last blank or the last label.
#pragma once
#include <math.h>

#include "common.h"

namespace tts {

constexpr int CTC_THREADS = 256;

// log(exp(a) + exp(b) + exp(c)) in fp64; -inf when all three are -inf
__device__ inline double lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// lab[0 .. 2n]; 1 in every thread for a target outside the symbols or the blank itself: no defined loss (two barriers; bad: one
// int of LDS)
__device__ __forceinline__ int ctc_extended_labels(int* lab, const int* __restrict__ targets, int n, int n_sym, int blank, int* bad) {
  if (threadIdx.x == 0) *bad = 0;
  __syncthreads();
  for (int s = threadIdx.x; s < 2 * n + 1; s += CTC_THREADS) {
    int v = blank;
    if (s & 1) {
      v = targets[s >> 1];
      if (v < 0 || v >= n_sym || v == blank) *bad = 1;  // (benign race: every writer stores 1)
      else if (s >= 3 && targets[(s >> 1) - 1] != v) v |= INT32_MIN;
    }
    lab[s] = v;
  }
  __syncthreads();
  return *bad;
}

// one wavefront: out[0 .. n_sym) = log_softmax of the row xr
__device__ __forceinline__ void ctc_log_softmax_row(const float* __restrict__ xr, int n_sym, int lane, float* out) {
  float m = -INFINITY;
  for (int k = lane; k < n_sym; k += 64) m = fmaxf(m, xr[k]);
  m = wave_max(m);
  float s = 0.0f;
  for (int k = lane; k < n_sym; k += 64) s += expf(xr[k] - m);
  const float ls = logf(wave_sum(s));
  for (int k = lane; k < n_sym; k += 64) out[k] = (xr[k] - m) - ls;
}

// alpha of state s at frame 0 and at a later frame; lp: the frame's log-probabilities, prev: alpha of the frame before
__device__ __forceinline__ double ctc_alpha_init(const int* lab, int s, const float* lp) {
  return s < 2 ? (double)lp[lab[s] & 0x7fffffff] : -INFINITY;
}

__device__ __forceinline__ double ctc_alpha_step(const double* prev, const int* lab, int s, const float* lp) {
  const int v = lab[s];
  const double a = prev[s];
  const double bb = s >= 1 ? prev[s - 1] : -INFINITY;
  const double cc = v < 0 ? prev[s - 2] : -INFINITY;
  return lse3(a, bb, cc) + (double)lp[v & 0x7fffffff];
}

// prev: alpha of the last frame
__device__ __forceinline__ double ctc_log_likelihood(const double* prev, int S) {
  return S >= 2 ? lse3(prev[S - 1], prev[S - 2], -INFINITY) : prev[S - 1];
}

}  // namespace tts
