// Kernels of the corpus scorer (Utility/Scorer.py): the aligner's CTC loss (AlignmentScorer.score, :33-61, through Aligner.inference
// with return_ctc, Aligner.py:60,107) and the four teacher-forced losses of ToucanTTSLoss (TTSScorer.score, :108-150;
// ToucanTTSLoss.py:20-66).  The logits and the acoustic model's outputs come from the existing kernels and stage entries.
//
// Batch independence: one workgroup per utterance, and an arithmetic order that depends on that utterance alone, so a batch returns
// bit for bit what its utterances return one by one.  No atomics; no workgroup waits on another one.
#include <math.h>

#include "common.h"
#include "ctc_lattice.h"
#include "../../include/toucan_score.h"

namespace tts {

// ---- CTC: the forward variables of ctc_lattice.h, one workgroup per utterance --------------------------------------------------
// Frames are taken in chunks of CTC_CHUNK: first the four wavefronts compute the log-softmax of the chunk's rows side by side (no
// dependency between frames) into LDS, then the workgroup walks the chunk's frames one after the other, one barrier per frame.
// LDS: alpha [2][S] fp64 (double-buffered rows), the extended labels [S] int32, the chunk's log-probabilities
// [CTC_CHUNK][n_symbols] fp32.
constexpr int CTC_CHUNK = 32, CTC_MAX_SYMBOLS = 256;

__global__ __launch_bounds__(CTC_THREADS) void ctc_loss_kernel(const float* __restrict__ logits, int ld, int n_sym,
                                                               const int* __restrict__ frame_begin, const int* __restrict__ n_frames,
                                                               const int* __restrict__ targets, const int* __restrict__ target_begin,
                                                               const int* __restrict__ n_targets, int blank, int s_pad,
                                                               float* __restrict__ loss) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* alpha = reinterpret_cast<double*>(smem);                            // [2][s_pad]
  int* lab = reinterpret_cast<int*>(smem + (size_t)2 * s_pad * sizeof(double));  // [s_pad]
  float* lp = reinterpret_cast<float*>(lab + s_pad);                          // [CTC_CHUNK][n_sym]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = n_frames[b], n = n_targets[b], S = 2 * n + 1;
  const float* x0 = logits + (size_t)frame_begin[b] * ld;
  const int* tg = targets + target_begin[b];
  if (T <= 0) {  // nothing to align (the host refuses this; no defined loss)
    if (tid == 0) loss[b] = NAN;
    return;
  }
  __shared__ int bad;
  if (ctc_extended_labels(lab, tg, n, n_sym, blank, &bad)) {
    if (tid == 0) loss[b] = NAN;
    return;
  }
  double* prev = alpha;
  double* cur = alpha + s_pad;
  for (int c0 = 0; c0 < T; c0 += CTC_CHUNK) {
    const int nc = min(CTC_CHUNK, T - c0);
    for (int f = wv; f < nc; f += CTC_THREADS / 64) ctc_log_softmax_row(x0 + (size_t)(c0 + f) * ld, n_sym, lane, lp + f * n_sym);
    __syncthreads();
    for (int f = 0; f < nc; ++f) {
      const float* lpf = lp + f * n_sym;
      if (c0 + f == 0) {
        for (int s = tid; s < S; s += CTC_THREADS) cur[s] = ctc_alpha_init(lab, s, lpf);
      } else {
        for (int s = tid; s < S; s += CTC_THREADS) cur[s] = ctc_alpha_step(prev, lab, s, lpf);
      }
      __syncthreads();
      double* t = prev;
      prev = cur;
      cur = t;
    }
  }
  if (tid == 0) {
    const double nll = -ctc_log_likelihood(prev, S);
    loss[b] = isinf(nll) ? 0.0f : (float)(nll / (double)max(n, 1));  // zero_infinity; reduction "mean" at batch 1
  }
}

int ctc_loss(const float* logits, int ld, int n_sym, const int* frame_begin, const int* n_frames, const int* targets, const int* target_begin,
             const int* n_targets, int batch, int blank, int max_targets, float* loss, hipStream_t st) {
  TTS_CHECK_ARG(logits && frame_begin && n_frames && targets && target_begin && n_targets && loss, "ctc_loss: null pointer");
  TTS_CHECK_ARG(n_sym > 0 && n_sym <= CTC_MAX_SYMBOLS && ld >= n_sym && blank >= 0 && blank < n_sym && batch >= 0,
                "ctc_loss: %d symbols (1 .. %d), row stride %d, blank %d", n_sym, CTC_MAX_SYMBOLS, ld, blank);
  TTS_CHECK_ARG(max_targets >= 0 && max_targets <= TTS_CTC_MAX_TARGETS, "ctc_loss: max targets %d (0 .. %d)", max_targets, TTS_CTC_MAX_TARGETS);
  if (batch == 0) return TTS_OK;
  const int s_pad = (2 * max_targets + 1 + 1) / 2 * 2;  // (even: the label array after the fp64 rows stays 16-byte aligned)
  const size_t lds = (size_t)2 * s_pad * sizeof(double) + (size_t)s_pad * sizeof(int) + (size_t)CTC_CHUNK * n_sym * sizeof(float);
  TTS_CHECK_ARG(lds <= 160 * 1024, "ctc_loss: %zu bytes of LDS requested", lds);
  static unsigned long long lds_raised = 0;
  if (lds > 64 * 1024 && raise_lds_limit(reinterpret_cast<const void*>(ctc_loss_kernel), lds_raised) != hipSuccess) {
    set_error("ctc_loss: raising the dynamic LDS limit for %zu bytes failed", lds);
    return TTS_E_LAUNCH;
  }
  hipLaunchKernelGGL(ctc_loss_kernel, dim3(batch), dim3(CTC_THREADS), lds, st, logits, ld, n_sym, frame_begin, n_frames, targets, target_begin,
                     n_targets, blank, s_pad, loss);
  return launch_status("ctc_loss");
}

// ---- the four losses of ToucanTTSLoss at batch 1, one workgroup per utterance ------------------------------------------------
// Each thread accumulates a fixed, strided subset of the utterance's elements in fp64; the 256 partial sums are added by a
// fixed-order tree.  The element differences are fp32, as in the reference (L1Loss / MSELoss on fp32 tensors).
constexpr int LOSS_THREADS = 256;

__global__ __launch_bounds__(LOSS_THREADS) void score_losses_kernel(const float* __restrict__ before, int ld_b, const float* __restrict__ after,
                                                                    int ld_a, const float* __restrict__ gold, int ld_g,
                                                                    const int* __restrict__ frame_begin, const int* __restrict__ n_frames,
                                                                    const float* __restrict__ log_dur, const float* __restrict__ pitch,
                                                                    const float* __restrict__ energy, const int* __restrict__ gold_dur,
                                                                    const float* __restrict__ gold_pitch, const float* __restrict__ gold_energy,
                                                                    const int* __restrict__ phone_begin, const int* __restrict__ n_phones,
                                                                    float* __restrict__ out) {
  __shared__ double red[4][LOSS_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = n_frames[b], f0 = frame_begin[b], L = n_phones[b], p0 = phone_begin[b];
  double l1 = 0.0, dl = 0.0, pl = 0.0, el = 0.0;
  for (long long e = tid; e < (long long)T * 80; e += LOSS_THREADS) {
    const int r = f0 + (int)(e / 80), c = (int)(e % 80);
    const float g = gold[(size_t)r * ld_g + c];
    l1 += (double)fabsf(before[(size_t)r * ld_b + c] - g);
    l1 += (double)fabsf(after[(size_t)r * ld_a + c] - g);
  }
  for (int k = tid; k < L; k += LOSS_THREADS) {
    const int i = p0 + k;
    const float d = log_dur[i] - log_rn((float)gold_dur[i] + 1.0f);  // DurationPredictorLoss: log(target + offset), offset 1.0
    const float p = pitch[i] - gold_pitch[i];
    const float q = energy[i] - gold_energy[i];
    dl += (double)d * d;
    pl += (double)p * p;
    el += (double)q * q;
  }
  red[0][tid] = l1;
  red[1][tid] = dl;
  red[2][tid] = pl;
  red[3][tid] = el;
  __syncthreads();
  for (int o = LOSS_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o)
      for (int j = 0; j < 4; ++j) red[j][tid] += red[j][tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    out[4 * b + 0] = (float)(red[0][0] / ((double)T * 80.0));
    out[4 * b + 1] = (float)(red[1][0] / (double)L);
    out[4 * b + 2] = (float)(red[2][0] / (double)L);
    out[4 * b + 3] = (float)(red[3][0] / (double)L);
  }
}

int score_losses(const float* before, int ld_b, const float* after, int ld_a, const float* gold, int ld_g, const int* frame_begin, const int* n_frames,
                 const float* log_dur, const float* pitch, const float* energy, const int* gold_dur, const float* gold_pitch, const float* gold_energy,
                 const int* phone_begin, const int* n_phones, int batch, float* out, hipStream_t st) {
  TTS_CHECK_ARG(before && after && gold && frame_begin && n_frames && log_dur && pitch && energy && gold_dur && gold_pitch && gold_energy &&
                    phone_begin && n_phones && out,
                "score_losses: null pointer");
  TTS_CHECK_ARG(ld_b >= 80 && ld_a >= 80 && ld_g >= 80 && batch >= 0, "score_losses: row strides %d %d %d (>= 80)", ld_b, ld_a, ld_g);
  if (batch == 0) return TTS_OK;
  hipLaunchKernelGGL(score_losses_kernel, dim3(batch), dim3(LOSS_THREADS), 0, st, before, ld_b, after, ld_a, gold, ld_g, frame_begin, n_frames,
                     log_dur, pitch, energy, gold_dur, gold_pitch, gold_energy, phone_begin, n_phones, out);
  return launch_status("score_losses");
}

}  // namespace tts

extern "C" {
int tts_ctc_loss(const float* logits, int32_t ld, int32_t n_symbols, const int32_t* frame_begin, const int32_t* n_frames, const int32_t* targets,
                 const int32_t* target_begin, const int32_t* n_targets, int32_t batch, int32_t blank, int32_t max_targets, float* loss,
                 tts_stream_t stream) {
  return tts::ctc_loss(logits, ld, n_symbols, frame_begin, n_frames, targets, target_begin, n_targets, batch, blank, max_targets, loss,
                       reinterpret_cast<hipStream_t>(stream));
}
int tts_score_losses(const float* before, int32_t ld_before, const float* after, int32_t ld_after, const float* gold, int32_t ld_gold,
                     const int32_t* frame_begin, const int32_t* n_frames, const float* log_dur, const float* pitch, const float* energy,
                     const int32_t* gold_dur, const float* gold_pitch, const float* gold_energy, const int32_t* phone_begin,
                     const int32_t* n_phones, int32_t batch, float* out, tts_stream_t stream) {
  return tts::score_losses(before, ld_before, after, ld_after, gold, ld_gold, frame_begin, n_frames, log_dur, pitch, energy, gold_dur, gold_pitch,
                           gold_energy, phone_begin, n_phones, batch, out, reinterpret_cast<hipStream_t>(stream));
}
}
