// Kernels of the aligner's on-line fine-tuning (InferenceInterfaces/UtteranceCloner.py:75-94): five SGD steps of CTC training of the
// Aligner (AutoAligner/Aligner.py:18-75) on one utterance - training-mode forward (BatchNorm with batch statistics, dropout),
// backward through all of it, clip_grad_norm_ and the SGD update.  finetune.py sequences them.
//
// fp32 throughout (the CTC recursions and the norm's partial sums fp64); every sum has a fixed order and there are no atomics, so a
// repeated call repeats its result bit for bit.  No workgroup waits on another one: the recurrences are one launch per time step.
#include <math.h>

#include "common.h"
#include "ctc_lattice.h"
#include "../../include/toucan_train.h"

namespace tts {

// ---- C (+)= op(A) op(B) on the fp32 matrix cores ----------------------------------------------------------------------------------
// Workgroup = a 64 x 64 tile of C, four wavefronts with one 32 x 32 accumulator each; K in chunks of 32 through LDS as As[k][m],
// Bs[k][n].  v_mfma_f32_32x32x2_f32 takes A[m = lane & 31][k = lane >> 5] and B[k = lane >> 5][n = lane & 31], so both operand reads
// are two runs of 32 consecutive words.  The row stride 97 (= 33 mod 64) is chosen by counting banks, not by measurement: of the
// 64 k-fastest stores a wavefront makes for a k-contiguous operand (k = 0 .. 31 at two neighbouring m) all but one pair fall on distinct
// banks (k = 31 at m and k = 0 at m + 1 meet), and an operand read's two runs (rows k and k + 1) overlap in one bank.  Elements outside M, N, K are loaded as zeros, so any size works (odd K included).
constexpr int GEMM_T = 64, GEMM_K = 32, GEMM_LD = 97;

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* C,
                                                       int ldc, const float* __restrict__ bias, int M, int N, int K, int accumulate) {
  __shared__ float As[GEMM_K][GEMM_LD];
  __shared__ float Bs[GEMM_K][GEMM_LD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m0 = blockIdx.y * GEMM_T, n0 = blockIdx.x * GEMM_T;
  const int wm = (wv >> 1) * 32, wn = (wv & 1) * 32;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int k0 = 0; k0 < K; k0 += GEMM_K) {
#pragma unroll
    for (int i = 0; i < GEMM_T * GEMM_K / 256; ++i) {
      const int idx = i * 256 + tid;
      {  // A: stored [m][k] (k contiguous) or, transposed, [k][m] (m contiguous): the threads run along the contiguous index
        const int k = TA ? idx >> 6 : idx & 31, m = TA ? idx & 63 : idx >> 5;
        const int gm = m0 + m, gk = k0 + k;
        float v = 0.0f;
        if (gm < M && gk < K) v = TA ? A[(size_t)gk * lda + gm] : A[(size_t)gm * lda + gk];
        As[k][m] = v;
      }
      {  // B: stored [k][n] or, transposed, [n][k]
        const int k = TB ? idx & 31 : idx >> 6, n = TB ? idx >> 5 : idx & 63;
        const int gn = n0 + n, gk = k0 + k;
        float v = 0.0f;
        if (gn < N && gk < K) v = TB ? B[(size_t)gn * ldb + gk] : B[(size_t)gk * ldb + gn];
        Bs[k][n] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GEMM_K; kk += 2) {
      const float a = As[kk + (lane >> 5)][wm + (lane & 31)];
      const float b = Bs[kk + (lane >> 5)][wn + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const int col = n0 + wn + (lane & 31);
  if (col >= N) return;
  const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < M) {
      float* cp = C + (size_t)row * ldc + col;
      float v = acc[r] + bv;
      if (accumulate) v += *cp;
      *cp = v;
    }
  }
}

int gemm_f32(int op, const float* a, int lda, const float* b, int ldb, float* c, int ldc, const float* bias, int m, int n, int k, int accumulate,
             hipStream_t st) {
  TTS_CHECK_ARG(op >= TTS_GEMM_NN && op <= TTS_GEMM_TN, "gemm_f32: op %d (0 NN, 1 NT, 2 TN)", op);
  TTS_CHECK_ARG(m >= 0 && n >= 0 && k >= 0 && lda > 0 && ldb > 0 && ldc >= n, "gemm_f32: sizes %d %d %d, leading dimensions %d %d %d", m, n, k,
                lda, ldb, ldc);
  if (m == 0 || n == 0) return TTS_OK;
  TTS_CHECK_ARG(c && (k == 0 || (a && b)), "gemm_f32: null pointer");
  const dim3 grid((n + GEMM_T - 1) / GEMM_T, (m + GEMM_T - 1) / GEMM_T);
  if (op == TTS_GEMM_NN)
    hipLaunchKernelGGL((gemm_f32_kernel<false, false>), grid, dim3(256), 0, st, a, lda, b, ldb, c, ldc, bias, m, n, k, accumulate);
  else if (op == TTS_GEMM_NT)
    hipLaunchKernelGGL((gemm_f32_kernel<false, true>), grid, dim3(256), 0, st, a, lda, b, ldb, c, ldc, bias, m, n, k, accumulate);
  else
    hipLaunchKernelGGL((gemm_f32_kernel<true, false>), grid, dim3(256), 0, st, a, lda, b, ldb, c, ldc, bias, m, n, k, accumulate);
  return launch_status("gemm_f32");
}

// ---- BatchNorm1d in training mode after the ReLU, with the dropout that follows ----------------------------------------------------
// Workgroup = 64 channels (lane = channel: a row of 64 channels is one 256-byte read) x 4 slices of the frames; the four partial
// sums of a channel are added in a fixed order.  Mean first, then the sum of squared deviations from it (two passes over r).
constexpr int BN_CH = 64, BN_SL = 4;

__device__ inline float bn_reduce(float v, float (*red)[BN_CH], int sl, int lane) {
  __syncthreads();  // the previous reduction's readers are done
  red[sl][lane] = v;
  __syncthreads();
  return (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ __launch_bounds__(256) void bn_train_forward_kernel(const float* __restrict__ z, int ldz, const uint8_t* __restrict__ mask,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* running_mean, float* running_var, float* __restrict__ y, int ldy,
                                                               float* __restrict__ save_mean, float* __restrict__ save_istd, int T, int C,
                                                               float eps, float momentum) {
  __shared__ float red[BN_SL][BN_CH];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6, c = blockIdx.x * BN_CH + lane;  // c < C: C is a multiple of 64
  float s = 0.0f;
  for (int t = sl; t < T; t += BN_SL) s += fmaxf(z[(size_t)t * ldz + c], 0.0f);
  const float mean = bn_reduce(s, red, sl, lane) / (float)T;
  float q = 0.0f;
  for (int t = sl; t < T; t += BN_SL) {
    const float d = fmaxf(z[(size_t)t * ldz + c], 0.0f) - mean;
    q = fmaf(d, d, q);
  }
  const float ssd = bn_reduce(q, red, sl, lane);
  const float var = ssd / (float)T;
  const float istd = 1.0f / sqrtf(var + eps);
  const float g = gamma[c], b = beta[c];
  for (int t = sl; t < T; t += BN_SL) {
    const float v = (fmaxf(z[(size_t)t * ldz + c], 0.0f) - mean) * istd * g + b;
    const float keep = mask ? (mask[(size_t)t * C + c] ? 2.0f : 0.0f) : 1.0f;
    y[(size_t)t * ldy + c] = v * keep;
  }
  if (sl == 0) {
    save_mean[c] = mean;
    save_istd[c] = istd;
    if (running_mean) running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
    if (running_var) running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (ssd / (float)(T - 1));
  }
}

__global__ __launch_bounds__(256) void bn_train_backward_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ z, int ldz,
                                                                const uint8_t* __restrict__ mask, const float* __restrict__ gamma,
                                                                const float* __restrict__ save_mean, const float* __restrict__ save_istd,
                                                                float* __restrict__ dz, int lddz, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, int T, int C) {
  __shared__ float red[BN_SL][BN_CH];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6, c = blockIdx.x * BN_CH + lane;
  const float mean = save_mean[c], istd = save_istd[c];
  float s1 = 0.0f, s2 = 0.0f;
  for (int t = sl; t < T; t += BN_SL) {
    const float keep = mask ? (mask[(size_t)t * C + c] ? 2.0f : 0.0f) : 1.0f;
    const float g = dy[(size_t)t * lddy + c] * keep;
    const float xh = (fmaxf(z[(size_t)t * ldz + c], 0.0f) - mean) * istd;
    s1 += g;
    s2 = fmaf(g, xh, s2);
  }
  s1 = bn_reduce(s1, red, sl, lane);
  s2 = bn_reduce(s2, red, sl, lane);
  const float m1 = s1 / (float)T, m2 = s2 / (float)T, k = gamma[c] * istd;
  for (int t = sl; t < T; t += BN_SL) {
    const float zv = z[(size_t)t * ldz + c];
    const float keep = mask ? (mask[(size_t)t * C + c] ? 2.0f : 0.0f) : 1.0f;
    const float g = dy[(size_t)t * lddy + c] * keep;
    const float xh = (fmaxf(zv, 0.0f) - mean) * istd;
    dz[(size_t)t * lddz + c] = zv > 0.0f ? k * (g - m1 - xh * m2) : 0.0f;
  }
  if (sl == 0) {
    dbeta[c] = s1;
    dgamma[c] = s2;
  }
}

__global__ void bn_eval_affine_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rm,
                                      const float* __restrict__ rv, float* __restrict__ scale, float* __restrict__ shift, int C, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double s = (double)gamma[c] / sqrt((double)rv[c] + (double)eps);
  scale[c] = (float)s;
  shift[c] = (float)((double)beta[c] - (double)rm[c] * s);
}

int bn_train_forward(const float* z, int ldz, const uint8_t* mask, const float* gamma, const float* beta, float* rm, float* rv, float* y, int ldy,
                     float* save_mean, float* save_istd, int T, int C, float eps, float momentum, hipStream_t st) {
  TTS_CHECK_ARG(z && gamma && beta && y && save_mean && save_istd, "bn_train_forward: null pointer");
  TTS_CHECK_ARG(C > 0 && C % BN_CH == 0 && ldz >= C && ldy >= C, "bn_train_forward: %d channels (a multiple of %d), strides %d %d", C, BN_CH, ldz, ldy);
  TTS_CHECK_ARG(T >= 2, "bn_train_forward: %d frames (training BatchNorm needs at least 2 values per channel)", T);
  hipLaunchKernelGGL(bn_train_forward_kernel, dim3(C / BN_CH), dim3(256), 0, st, z, ldz, mask, gamma, beta, rm, rv, y, ldy, save_mean, save_istd, T,
                     C, eps, momentum);
  return launch_status("bn_train_forward");
}

int bn_train_backward(const float* dy, int lddy, const float* z, int ldz, const uint8_t* mask, const float* gamma, const float* save_mean,
                      const float* save_istd, float* dz, int lddz, float* dgamma, float* dbeta, int T, int C, hipStream_t st) {
  TTS_CHECK_ARG(dy && z && gamma && save_mean && save_istd && dz && dgamma && dbeta && dz != dy, "bn_train_backward: null or aliased pointer");
  TTS_CHECK_ARG(C > 0 && C % BN_CH == 0 && lddy >= C && ldz >= C && lddz >= C && T >= 2, "bn_train_backward: %d channels, %d frames", C, T);
  hipLaunchKernelGGL(bn_train_backward_kernel, dim3(C / BN_CH), dim3(256), 0, st, dy, lddy, z, ldz, mask, gamma, save_mean, save_istd, dz, lddz,
                     dgamma, dbeta, T, C);
  return launch_status("bn_train_backward");
}

int bn_eval_affine(const float* gamma, const float* beta, const float* rm, const float* rv, float* scale, float* shift, int C, float eps,
                   hipStream_t st) {
  TTS_CHECK_ARG(gamma && beta && rm && rv && scale && shift && C > 0, "bn_eval_affine: bad arguments");
  hipLaunchKernelGGL(bn_eval_affine_kernel, dim3((C + 255) / 256), dim3(256), 0, st, gamma, beta, rm, rv, scale, shift, C, eps);
  return launch_status("bn_eval_affine");
}

// ---- the bidirectional LSTM, one launch per time step ------------------------------------------------------------------------------
// Forward step.  Workgroup (slice of 4 hidden units, direction): its 16 gate rows of W_hh (row = gate*H + unit) times h of the
// previous step; 256 threads = 16 rows x 16 interleaved slices of k (16 consecutive lanes read 16 consecutive words of a row).  The
// 16 partial sums of a row are added in a fixed order.  Unlike tts_lstm_recurrence it reads W_hh as torch stores it (the weights
// change on the device every step) and keeps the activated gates and the cell state of every step.
constexpr int LT_UNITS = 4, LT_KS = 16;

template <int H>
__global__ __launch_bounds__(256) void lstm_train_step_kernel(const float* __restrict__ xproj, int ldx, const float* __restrict__ w_hh,
                                                              const float* __restrict__ b_ih, const float* __restrict__ b_hh, float* y, int ldy,
                                                              float* __restrict__ gates, float* cseq, int T, int step) {
  __shared__ float hs[H];
  __shared__ float red[LT_KS][LT_UNITS * 4];
  const int tid = threadIdx.x, ks = tid & 15, col = tid >> 4;  // col = gate*4 + unit
  const int dir = blockIdx.y, u0 = blockIdx.x * LT_UNITS;
  const int row = dir == 0 ? step : T - 1 - step, row_prev = dir == 0 ? step - 1 : T - step;
  for (int k = tid; k < H; k += 256) hs[k] = step > 0 ? y[(size_t)row_prev * ldy + dir * H + k] : 0.0f;
  __syncthreads();
  const float* wr = w_hh + ((size_t)dir * 4 * H + (size_t)(col >> 2) * H + u0 + (col & 3)) * H;
  float a = 0.0f;
#pragma unroll 8
  for (int kk = 0; kk < H / LT_KS; ++kk) a = fmaf(wr[kk * LT_KS + ks], hs[kk * LT_KS + ks], a);
  red[ks][col] = a;
  __syncthreads();
  if (tid < LT_UNITS) {
    const int u = u0 + tid;
    float g4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float s = 0.0f;
      for (int q = 0; q < LT_KS; ++q) s += red[q][g * 4 + tid];
      const int m = dir * 4 * H + g * H + u;
      g4[g] = (xproj[(size_t)row * ldx + m] + (b_ih[m] + b_hh[m])) + s;
    }
    const float ig = 1.0f / (1.0f + expf(-g4[0]));  // PyTorch's gate order i, f, g, o
    const float fg = 1.0f / (1.0f + expf(-g4[1]));
    const float gg = tanhf(g4[2]);
    const float og = 1.0f / (1.0f + expf(-g4[3]));
    const float cp = step > 0 ? cseq[((size_t)row_prev * 2 + dir) * H + u] : 0.0f;
    const float c = fg * cp + ig * gg;
    float* gr = gates + ((size_t)row * 2 + dir) * 4 * H + u;
    gr[0] = ig;
    gr[H] = fg;
    gr[2 * H] = gg;
    gr[3 * H] = og;
    cseq[((size_t)row * 2 + dir) * H + u] = c;
    y[(size_t)row * ldy + dir * H + u] = og * tanhf(c);
  }
}

// Backward step.  Workgroup (slice of 16 hidden units, direction): dh = dy + W_hh^T dgates(next step), the latter as 16 columns of
// W_hh (16 consecutive lanes read 16 consecutive words of a row) x 16 interleaved slices of the 4H gate rows; then the gate
// derivatives of its 16 units.  The cell gradient of a unit is carried in dc by the workgroup that owns the unit.
constexpr int LB_UNITS = 16, LB_MS = 16;

template <int H>
__global__ __launch_bounds__(256) void lstm_backward_step_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ w_hh,
                                                                 const float* __restrict__ gates, const float* __restrict__ cseq, float* dgates,
                                                                 float* dc, int T, int step) {
  __shared__ float dgs[4 * H];
  __shared__ float red[LB_MS][LB_UNITS];
  const int tid = threadIdx.x, u = tid & 15, ms = tid >> 4;
  const int dir = blockIdx.y, j = blockIdx.x * LB_UNITS + u;
  const int row = dir == 0 ? step : T - 1 - step;
  const int row_next = dir == 0 ? step + 1 : T - 2 - step, row_prev = dir == 0 ? step - 1 : T - step;
  const bool last = step == T - 1;  // the first call: nothing flows back yet (uniform)
  float a = 0.0f;
  if (!last) {
    const float* dgn = dgates + ((size_t)row_next * 2 + dir) * 4 * H;
    for (int m = tid; m < 4 * H; m += 256) dgs[m] = dgn[m];
    __syncthreads();
    const float* wc = w_hh + (size_t)dir * 4 * H * H + j;
#pragma unroll 8
    for (int q = 0; q < 4 * H / LB_MS; ++q) {
      const int m = q * LB_MS + ms;
      a = fmaf(wc[(size_t)m * H], dgs[m], a);
    }
  }
  red[ms][u] = a;
  __syncthreads();
  if (tid < LB_UNITS) {
    float rec = 0.0f;
    for (int q = 0; q < LB_MS; ++q) rec += red[q][u];
    const float dh = dy[(size_t)row * lddy + dir * H + j] + rec;
    const float* gr = gates + ((size_t)row * 2 + dir) * 4 * H + j;
    const float ig = gr[0], fg = gr[H], gg = gr[2 * H], og = gr[3 * H];
    const float c = cseq[((size_t)row * 2 + dir) * H + j];
    const float cp = step > 0 ? cseq[((size_t)row_prev * 2 + dir) * H + j] : 0.0f;
    const float tc = tanhf(c);
    const float dcv = (last ? 0.0f : dc[dir * H + j]) + dh * og * (1.0f - tc * tc);
    float* dg = dgates + ((size_t)row * 2 + dir) * 4 * H + j;
    dg[0] = dcv * gg * ig * (1.0f - ig);
    dg[H] = dcv * cp * fg * (1.0f - fg);
    dg[2 * H] = dcv * ig * (1.0f - gg * gg);
    dg[3 * H] = dh * tc * og * (1.0f - og);
    dc[dir * H + j] = dcv * fg;
  }
}

int lstm_train_step(const float* xproj, int ldx, const float* w_hh, const float* b_ih, const float* b_hh, float* y, int ldy, float* gates,
                    float* cseq, int T, int hidden, int step, hipStream_t st) {
  TTS_CHECK_ARG(xproj && w_hh && b_ih && b_hh && y && gates && cseq, "lstm_train_step: null pointer");
  TTS_CHECK_ARG(hidden == 512, "lstm_train_step: hidden %d (512)", hidden);
  TTS_CHECK_ARG(ldx >= 8 * hidden && ldy >= 2 * hidden && T >= 1 && step >= 0 && step < T, "lstm_train_step: strides %d %d, step %d of %d", ldx,
                ldy, step, T);
  hipLaunchKernelGGL(lstm_train_step_kernel<512>, dim3(512 / LT_UNITS, 2), dim3(256), 0, st, xproj, ldx, w_hh, b_ih, b_hh, y, ldy, gates, cseq, T,
                     step);
  return launch_status("lstm_train_step");
}

int lstm_backward_step(const float* dy, int lddy, const float* w_hh, const float* gates, const float* cseq, float* dgates, float* dc, int T,
                       int hidden, int step, hipStream_t st) {
  TTS_CHECK_ARG(dy && w_hh && gates && cseq && dgates && dc, "lstm_backward_step: null pointer");
  TTS_CHECK_ARG(hidden == 512, "lstm_backward_step: hidden %d (512)", hidden);
  TTS_CHECK_ARG(lddy >= 2 * hidden && T >= 1 && step >= 0 && step < T, "lstm_backward_step: stride %d, step %d of %d", lddy, step, T);
  hipLaunchKernelGGL(lstm_backward_step_kernel<512>, dim3(512 / LB_UNITS, 2), dim3(256), 0, st, dy, lddy, w_hh, gates, cseq, dgates, dc, T, step);
  return launch_status("lstm_backward_step");
}

// ---- CTC loss and its gradient with respect to the logits, one workgroup -----------------------------------------------------------
// The lattice of ctc_lattice.h.  Pass 1: the log-softmax of every frame into lp (the four wavefronts side by side).  Pass 2: the
// forward variables alpha, two rows in LDS and every row to global scratch.  Pass 3, frames backwards: the backward
// variables beta (two rows in LDS); per state the posterior exp(alpha + beta - lp - ll) into LDS; then one thread per symbol adds
// the posteriors of the symbol's states along a list (first[k], next[s]: ascending s, a fixed order) and writes
// grad = (softmax - posterior) / n.  The state loops run in strides of the workgroup, so S may exceed 256.
constexpr int CG_THREADS = CTC_THREADS, CG_MAX_SYMBOLS = 256;

__global__ __launch_bounds__(CG_THREADS) void ctc_grad_kernel(const float* __restrict__ logits, int ld, int n_sym, int T,
                                                              const int* __restrict__ targets, int n, int blank, double* __restrict__ alpha,
                                                              float* __restrict__ lp, float* __restrict__ loss, float* __restrict__ grad, int ldg,
                                                              int s_pad) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* rows = reinterpret_cast<double*>(smem);           // [2][s_pad]: alpha, then beta
  double* post = rows + (size_t)2 * s_pad;                  // [s_pad]
  int* lab = reinterpret_cast<int*>(post + s_pad);          // [s_pad]; bit 31: the skip s-2 -> s is allowed
  int* next = lab + s_pad;                                  // [s_pad]
  __shared__ int first[CG_MAX_SYMBOLS];
  __shared__ int bad;
  __shared__ double ll_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, S = 2 * n + 1;
  if (ctc_extended_labels(lab, targets, n, n_sym, blank, &bad)) {  // no defined loss: report, as tts_ctc_loss does
    if (tid == 0) loss[0] = NAN;
    for (int i = tid; i < T * n_sym; i += CG_THREADS) grad[(size_t)(i / n_sym) * ldg + i % n_sym] = NAN;
    return;
  }
  // per symbol the ascending list of its states
  if (tid < n_sym) {
    int prev = -1;
    first[tid] = -1;
    for (int s = 0; s < S; ++s) {
      if ((lab[s] & 0x7fffffff) != tid) continue;
      if (prev < 0) first[tid] = s;
      else next[prev] = s;
      prev = s;
    }
    if (prev >= 0) next[prev] = -1;
  }
  // pass 1
  for (int t = wv; t < T; t += CG_THREADS / 64) ctc_log_softmax_row(logits + (size_t)t * ld, n_sym, lane, lp + (size_t)t * n_sym);
  __syncthreads();  // lp is read below by other threads of this workgroup than wrote it
  // pass 2: alpha
  double* prev = rows;
  double* cur = rows + s_pad;
  for (int t = 0; t < T; ++t) {
    const float* lpt = lp + (size_t)t * n_sym;
    for (int s = tid; s < S; s += CG_THREADS) {
      const double a = t == 0 ? ctc_alpha_init(lab, s, lpt) : ctc_alpha_step(prev, lab, s, lpt);
      cur[s] = a;
      alpha[(size_t)t * S + s] = a;
    }
    __syncthreads();
    double* tmp = prev;
    prev = cur;
    cur = tmp;
  }
  if (tid == 0) ll_s = ctc_log_likelihood(prev, S);
  __syncthreads();
  const double ll = ll_s;
  const double inv_n = 1.0 / (double)n;
  if (ll == -INFINITY) {  // zero_infinity: loss 0, gradient 0 (uniform branch)
    if (tid == 0) loss[0] = 0.0f;
    for (int i = tid; i < T * n_sym; i += CG_THREADS) grad[(size_t)(i / n_sym) * ldg + i % n_sym] = 0.0f;
    return;
  }
  if (tid == 0) loss[0] = (float)(-ll * inv_n);
  // pass 3: beta, posteriors, gradient
  for (int t = T - 1; t >= 0; --t) {
    const float* lpt = lp + (size_t)t * n_sym;
    for (int s = tid; s < S; s += CG_THREADS) {
      const double l = (double)lpt[lab[s] & 0x7fffffff];
      double b;
      if (t == T - 1) {
        b = s >= S - 2 ? l : -INFINITY;
      } else {
        const double bb = s + 1 < S ? prev[s + 1] : -INFINITY;
        const double cc = (s + 2 < S && lab[s + 2] < 0) ? prev[s + 2] : -INFINITY;
        b = lse3(prev[s], bb, cc) + l;
      }
      cur[s] = b;
      post[s] = exp(alpha[(size_t)t * S + s] + b - l - ll);  // alpha and beta both hold this frame's lp; exp(-inf) = 0
    }
    __syncthreads();
    if (tid < n_sym) {
      double p = 0.0;
      for (int s = first[tid]; s >= 0; s = next[s]) p += post[s];
      grad[(size_t)t * ldg + tid] = (float)((exp((double)lpt[tid]) - p) * inv_n);
    }
    __syncthreads();  // post is rewritten next frame
    double* tmp = prev;
    prev = cur;
    cur = tmp;
  }
}

int ctc_grad(const float* logits, int ld, int n_sym, int T, const int* targets, int n, int blank, double* alpha, float* lp, float* loss,
             float* grad, int ldg, hipStream_t st) {
  TTS_CHECK_ARG(logits && targets && alpha && lp && loss && grad, "ctc_grad: null pointer");
  TTS_CHECK_ARG(n_sym > 0 && n_sym <= CG_MAX_SYMBOLS && ld >= n_sym && ldg >= n_sym && blank >= 0 && blank < n_sym && T >= 1,
                "ctc_grad: %d symbols (1 .. %d), strides %d %d, blank %d, %d frames", n_sym, CG_MAX_SYMBOLS, ld, ldg, blank, T);
  TTS_CHECK_ARG(n >= 1 && n <= TTS_CTC_GRAD_MAX_TARGETS, "ctc_grad: %d targets (1 .. %d)", n, TTS_CTC_GRAD_MAX_TARGETS);
  const int s_pad = (2 * n + 1 + 1) / 2 * 2;
  const size_t lds = (size_t)3 * s_pad * sizeof(double) + (size_t)2 * s_pad * sizeof(int);  // 49 216 bytes at the 768-target cap, beside 1 KiB of static LDS: inside the 64 KiB a workgroup has without raising the limit
  hipLaunchKernelGGL(ctc_grad_kernel, dim3(1), dim3(CG_THREADS), lds, st, logits, ld, n_sym, T, targets, n, blank, alpha, lp, loss, grad, ldg,
                     s_pad);
  return launch_status("ctc_grad");
}

// ---- column sums, the gradient norm, the update -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void col_sum_kernel(const float* __restrict__ x, int ldx, int rows, int cols, float* __restrict__ out,
                                                      float* __restrict__ out2) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  float s = 0.0f;
  if (c < cols)
    for (int r = sl; r < rows; r += 4) s += x[(size_t)r * ldx + c];
  red[sl][lane] = s;
  __syncthreads();
  if (sl == 0 && c < cols) {
    const float v = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    out[c] = v;
    if (out2) out2[c] = v;
  }
}

int col_sum(const float* x, int ldx, int rows, int cols, float* out, float* out2, hipStream_t st) {
  TTS_CHECK_ARG(x && out && rows >= 0 && cols > 0 && ldx >= cols, "col_sum: bad arguments");
  hipLaunchKernelGGL(col_sum_kernel, dim3((cols + 63) / 64), dim3(256), 0, st, x, ldx, rows, cols, out, out2);
  return launch_status("col_sum");
}

// the 256 values in the LDS tree's order (wave_ops.h block_tree_fold: not the butterfly's)
__device__ inline double tree_sum(double v, double* red) {
  return block_tree_fold(v, red, [](double a, double b) { return a + b; });
}

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, long long n, double* __restrict__ partials) {
  __shared__ double red[256];
  const long long chunk = (n + TTS_SUMSQ_PARTIALS - 1) / TTS_SUMSQ_PARTIALS;
  const long long b = (long long)blockIdx.x * chunk, e = b + chunk < n ? b + chunk : n;
  double s = 0.0;
  for (long long i = b + threadIdx.x; i < e; i += 256) s += (double)x[i] * (double)x[i];
  s = tree_sum(s, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sumsq_final_kernel(const double* __restrict__ partials, float* __restrict__ norm) {
  __shared__ double red[256];
  const double s = tree_sum(partials[threadIdx.x], red);
  if (threadIdx.x == 0) norm[0] = (float)sqrt(s);
}

int sumsq(const float* x, long long n, double* partials, float* norm, hipStream_t st) {
  TTS_CHECK_ARG(x && partials && norm && n >= 0, "sumsq: bad arguments");
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(TTS_SUMSQ_PARTIALS), dim3(256), 0, st, x, n, partials);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, st, partials, norm);
  return launch_status("sumsq");
}

__global__ void sgd_clip_update_kernel(float* __restrict__ p, const float* __restrict__ g, long long n, const float* __restrict__ norm,
                                       float max_norm, float lr) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float coef = fminf(max_norm / (norm[0] + 1.0e-6f), 1.0f);
  p[i] = p[i] - lr * (g[i] * coef);
}

int sgd_clip_update(float* p, const float* g, long long n, const float* norm, float max_norm, float lr, hipStream_t st) {
  TTS_CHECK_ARG(p && g && norm && n >= 0 && max_norm > 0.0f, "sgd_clip_update: bad arguments");
  if (n == 0) return TTS_OK;
  hipLaunchKernelGGL(sgd_clip_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, g, n, norm, max_norm, lr);
  return launch_status("sgd_clip_update");
}

}  // namespace tts

extern "C" {
int tts_gemm_f32(int32_t op, const float* a, int32_t lda, const float* b, int32_t ldb, float* c, int32_t ldc, const float* bias, int32_t m,
                 int32_t n, int32_t k, int32_t accumulate, tts_stream_t stream) {
  return tts::gemm_f32(op, a, lda, b, ldb, c, ldc, bias, m, n, k, accumulate, reinterpret_cast<hipStream_t>(stream));
}
int tts_bn_train_forward(const float* z, int32_t ldz, const uint8_t* mask, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float* y, int32_t ldy, float* save_mean, float* save_istd, int32_t t, int32_t c, float eps,
                         float momentum, tts_stream_t stream) {
  return tts::bn_train_forward(z, ldz, mask, gamma, beta, running_mean, running_var, y, ldy, save_mean, save_istd, t, c, eps, momentum,
                               reinterpret_cast<hipStream_t>(stream));
}
int tts_bn_train_backward(const float* dy, int32_t lddy, const float* z, int32_t ldz, const uint8_t* mask, const float* gamma,
                          const float* save_mean, const float* save_istd, float* dz, int32_t lddz, float* dgamma, float* dbeta, int32_t t,
                          int32_t c, tts_stream_t stream) {
  return tts::bn_train_backward(dy, lddy, z, ldz, mask, gamma, save_mean, save_istd, dz, lddz, dgamma, dbeta, t, c,
                                reinterpret_cast<hipStream_t>(stream));
}
int tts_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float* scale,
                       float* shift, int32_t c, float eps, tts_stream_t stream) {
  return tts::bn_eval_affine(gamma, beta, running_mean, running_var, scale, shift, c, eps, reinterpret_cast<hipStream_t>(stream));
}
int tts_lstm_train_step(const float* xproj, int32_t ldx, const float* w_hh, const float* b_ih, const float* b_hh, float* y, int32_t ldy,
                        float* gates, float* cseq, int32_t t, int32_t hidden, int32_t step, tts_stream_t stream) {
  return tts::lstm_train_step(xproj, ldx, w_hh, b_ih, b_hh, y, ldy, gates, cseq, t, hidden, step, reinterpret_cast<hipStream_t>(stream));
}
int tts_lstm_backward_step(const float* dy, int32_t lddy, const float* w_hh, const float* gates, const float* cseq, float* dgates, float* dc,
                           int32_t t, int32_t hidden, int32_t step, tts_stream_t stream) {
  return tts::lstm_backward_step(dy, lddy, w_hh, gates, cseq, dgates, dc, t, hidden, step, reinterpret_cast<hipStream_t>(stream));
}
int tts_ctc_grad(const float* logits, int32_t ld, int32_t n_symbols, int32_t t, const int32_t* targets, int32_t n_targets, int32_t blank,
                 double* alpha, float* lp, float* loss, float* grad, int32_t ldg, tts_stream_t stream) {
  return tts::ctc_grad(logits, ld, n_symbols, t, targets, n_targets, blank, alpha, lp, loss, grad, ldg, reinterpret_cast<hipStream_t>(stream));
}
int tts_col_sum(const float* x, int32_t ldx, int32_t rows, int32_t cols, float* out, float* out2, tts_stream_t stream) {
  return tts::col_sum(x, ldx, rows, cols, out, out2, reinterpret_cast<hipStream_t>(stream));
}
int tts_sumsq(const float* x, int64_t n, double* partials, float* norm, tts_stream_t stream) {
  return tts::sumsq(x, (long long)n, partials, norm, reinterpret_cast<hipStream_t>(stream));
}
int tts_sgd_clip_update(float* p, const float* g, int64_t n, const float* norm, float max_norm, float lr, tts_stream_t stream) {
  return tts::sgd_clip_update(p, g, (long long)n, norm, max_norm, lr, reinterpret_cast<hipStream_t>(stream));
}
}
