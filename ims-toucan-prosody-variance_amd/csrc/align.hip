// Kernels of the prosody cloner (InferenceInterfaces/UtteranceCloner.py:46-145): the parts of the Aligner that are not dense products
// (TrainingInterfaces/Text_to_Spectrogram/AutoAligner/Aligner.py:18-75 - eval BatchNorm after the ReLU, the recurrence of the
// bidirectional LSTM), monotonic alignment search with the duration post-processing of extract_prosody (Aligner.py:202-234,
// DurationCalculator.py, UtteranceCloner.py:95-131), frame energy (EnergyCalculator.py:38-93) and the token averages of energy and
// pitch (EnergyCalculator.py:73-84, PitchCalculator.py:106-117).  The convs, the LSTM input projection and the output projection are
// dense products and run through tts_conv1d (align.py packs them).  fp32 throughout: durations come out of an argmax path.
//
// Batch independence: every kernel here computes an utterance with an arithmetic order that depends on that utterance alone, so a
// batch returns bit for bit what the utterances return one by one.  No workgroup waits on another one.
#include "common.h"
#include "../../include/toucan_align.h"

namespace tts {

// ---- BatchNorm(eval) after ReLU: y = relu(x) * scale[c] + shift[c]   (BatchNormConv.forward, Aligner.py:28-34) -------------------
__global__ void relu_affine_kernel(const float* x, int ldx, float* y, int ldy, int rows, int c,
                                   const float* __restrict__ scale, const float* __restrict__ shift) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)rows * c) return;
  const int r = (int)(i / c), k = (int)(i % c);
  y[(size_t)r * ldy + k] = fmaxf(x[(size_t)r * ldx + k], 0.0f) * scale[k] + shift[k];
}

int relu_affine(const float* x, int ldx, float* y, int ldy, int rows, int c, const float* scale, const float* shift, hipStream_t st) {
  TTS_CHECK_ARG(x && y && scale && shift && rows >= 0 && c > 0 && ldx >= c && ldy >= c, "relu_affine: bad arguments");
  if (rows == 0) return TTS_OK;
  const long long n = (long long)rows * c;
  hipLaunchKernelGGL(relu_affine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, ldx, y, ldy, rows, c, scale, shift);
  return launch_status("relu_affine");
}

// ---- one time step of a bidirectional LSTM on a ragged packed batch ------------------------------------------------------------
// Workgroup (unit slice, direction, chunk of LSTM_NB utterances): 4 hidden units and their 4 gates = 16 gate columns; 256 threads =
// 16 columns (column = gate*4 + unit) x 16 slices of the hidden input (KPT values each, in registers).  The partial products of the 16 slices are summed in
// LDS in a fixed order, so an utterance's result does not depend on the batch or on the chunk it falls in.  The input projection
// and the cell state of the step are requested before the products, so their latency hides behind them.
constexpr int LSTM_UNITS = 4, LSTM_KG = 16, LSTM_NB = 8;

template <int KPT>
__global__ __launch_bounds__(256) void lstm_step_kernel(const float* __restrict__ xproj, int ldx, const float* __restrict__ w_hh_blk,
                                                        const float* __restrict__ h_in, const float* __restrict__ c_in,
                                                        float* __restrict__ h_out, float* __restrict__ c_out, float* __restrict__ y, int ldy,
                                                        const int* __restrict__ seq_begin, const int* __restrict__ seq_len, int batch,
                                                        int step) {
  constexpr int H = KPT * LSTM_KG;
  __shared__ float hs[LSTM_NB][H];
  __shared__ float red[LSTM_KG][LSTM_NB][LSTM_UNITS * 4];
  const int tid = threadIdx.x, col = tid & 15, kg = tid >> 4;
  const int dir = blockIdx.y, u0 = blockIdx.x * LSTM_UNITS, b0 = blockIdx.z * LSTM_NB;
  bool any = false;
  for (int nb = 0; nb < LSTM_NB; ++nb) any |= b0 + nb < batch && step < seq_len[b0 + nb];
  if (!any) return;  // every utterance of this chunk has ended (uniform across the workgroup)

  // the cell-update threads (one per utterance and unit) fetch the input projection and the cell state first
  const int nb_c = tid >> 2, u_c = tid & 3, b_c = b0 + nb_c;
  const bool upd = tid < LSTM_NB * LSTM_UNITS && b_c < batch && step < seq_len[b_c];
  float xg[4] = {0.f, 0.f, 0.f, 0.f}, cp = 0.0f;
  int row = 0;
  if (upd) {
    const int len = seq_len[b_c];
    row = seq_begin[b_c] + (dir == 0 ? step : len - 1 - step);  // the reverse direction starts at the utterance's own end
    const float* xr = xproj + (size_t)row * ldx + (size_t)dir * 4 * H + u0 + u_c;
#pragma unroll
    for (int g = 0; g < 4; ++g) xg[g] = xr[g * H];
    if (step > 0) cp = c_in[((size_t)b_c * 2 + dir) * H + u0 + u_c];
  }
  // W_hh blocked per unit slice [dir][slice][kk][kg][col] (k = kg*KPT + kk): for each kk the workgroup reads 1 KiB in one piece
  float w[KPT];
  const float* wp = w_hh_blk + ((size_t)dir * (H / LSTM_UNITS) + blockIdx.x) * (size_t)H * 16 + tid;
#pragma unroll
  for (int kk = 0; kk < KPT; ++kk) w[kk] = wp[(size_t)kk * 256];
  // the hidden states of this chunk; the first step starts from zero and never reads h_in
  for (int i = tid; i < LSTM_NB * H; i += 256) {
    const int nb = i / H, k = i % H, b = b0 + nb;
    float v = 0.0f;
    if (step > 0 && b < batch && step < seq_len[b]) v = h_in[((size_t)b * 2 + dir) * H + k];
    hs[nb][k] = v;
  }
  __syncthreads();
#pragma unroll
  for (int nb = 0; nb < LSTM_NB; ++nb) {
    float a = 0.0f;
#pragma unroll
    for (int kk = 0; kk < KPT; ++kk) a = fmaf(w[kk], hs[nb][kg * KPT + kk], a);
    red[kg][nb][col] = a;
  }
  __syncthreads();
  if (upd) {
    float g4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float s = 0.0f;
      for (int q = 0; q < LSTM_KG; ++q) s += red[q][nb_c][g * 4 + u_c];
      g4[g] = xg[g] + s;
    }
    // PyTorch's gate order i, f, g, o
    const float ig = 1.0f / (1.0f + expf(-g4[0]));
    const float fg = 1.0f / (1.0f + expf(-g4[1]));
    const float gg = tanhf(g4[2]);
    const float og = 1.0f / (1.0f + expf(-g4[3]));
    const float c = fg * cp + ig * gg;
    const float h = og * tanhf(c);
    const size_t si = ((size_t)b_c * 2 + dir) * H + u0 + u_c;
    c_out[si] = c;
    h_out[si] = h;
    y[(size_t)row * ldy + (size_t)dir * H + u0 + u_c] = h;
  }
}

int lstm_step(const float* xproj, int ldx, const float* w_hh_blk, const float* h_in, const float* c_in, float* h_out, float* c_out, float* y,
              int ldy, const int* seq_begin, const int* seq_len, int batch, int hidden, int step, hipStream_t st) {
  TTS_CHECK_ARG(xproj && w_hh_blk && h_in && c_in && h_out && c_out && y && seq_begin && seq_len, "lstm_recurrence: null pointer");
  TTS_CHECK_ARG(hidden == 256 || hidden == 512, "lstm_recurrence: hidden %d (256 or 512)", hidden);
  TTS_CHECK_ARG(ldx >= 8 * hidden && ldy >= 2 * hidden && batch >= 0 && step >= 0, "lstm_recurrence: bad strides / sizes");
  TTS_CHECK_ARG(h_in != h_out && c_in != c_out, "lstm_recurrence: the state buffers must ping-pong");
  if (batch == 0) return TTS_OK;
  const dim3 grid(hidden / LSTM_UNITS, 2, (batch + LSTM_NB - 1) / LSTM_NB);
  if (hidden == 512)
    hipLaunchKernelGGL(lstm_step_kernel<32>, grid, dim3(256), 0, st, xproj, ldx, w_hh_blk, h_in, c_in, h_out, c_out, y, ldy, seq_begin, seq_len,
                       batch, step);
  else
    hipLaunchKernelGGL(lstm_step_kernel<16>, grid, dim3(256), 0, st, xproj, ldx, w_hh_blk, h_in, c_in, h_out, c_out, y, ldy, seq_begin, seq_len,
                       batch, step);
  return launch_status("lstm_recurrence");
}

// ---- MAS + DurationCalculator + the duration repair of extract_prosody, one workgroup per utterance ----------------------------
// LDS: two DP rows [lpad] f32, then the decision bits (lds_words 64-bit words), then nothing else; the durations are built in
// the output itself by thread 0.
constexpr int MAS_THREADS = 256;

static_assert(MAS_THREADS == 256, "block_tree_fold is a tree over 256 threads");

__global__ __launch_bounds__(MAS_THREADS) void mas_durations_kernel(const float* __restrict__ logits, int ld, const int* __restrict__ frame_begin,
                                                                    const int* __restrict__ n_frames, const int* __restrict__ ids,
                                                                    const int* __restrict__ id_begin, const int* __restrict__ n_ids,
                                                                    const int* __restrict__ flags, const int* __restrict__ full_begin,
                                                                    const int* __restrict__ n_full, const long long* __restrict__ scratch_off,
                                                                    unsigned long long* __restrict__ scratch, int lpad, int lds_words,
                                                                    int* __restrict__ durations) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ float red[MAS_THREADS];
  float* rows = reinterpret_cast<float*>(smem);  // [2][lpad]
  unsigned long long* lds_bits = reinterpret_cast<unsigned long long*>(smem + (size_t)2 * lpad * sizeof(float));
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = n_frames[b], L = n_ids[b], Lf = n_full[b], fb = frame_begin[b];
  const int* tok = ids + id_begin[b];
  int* out = durations + full_begin[b];
  const int* fl = flags + full_begin[b];
  const int W = (L + 63) / 64;  // 64-bit words per frame row
  const long long need = (long long)T * W;
  const long long off = scratch_off[b];
  __shared__ int n_words;  // non-boundary tokens of the full text: must be the L aligned tokens
  if (tid == 0) {
    int n = 0;
    for (int k = 0; k < Lf; ++k) n += (fl[k] & 1) ? 0 : 1;
    n_words = n;
  }
  __syncthreads();
  if (T <= 0 || L <= 0 || L > lpad || n_words != L || (off < 0 && need > lds_words)) {  // no layout for this utterance: report, touch nothing else
    for (int k = tid; k < Lf; k += MAS_THREADS) out[k] = -1;
    return;
  }
  unsigned long long* bits = off < 0 ? lds_bits : scratch + off;

  // M = max |p| over the token columns (Aligner.py:208); the reduction order does not matter for a maximum
  float m = 0.0f;
  for (long long c = tid; c < (long long)T * L; c += MAS_THREADS) {
    const int i = (int)(c / L), j = (int)(c % L);
    m = fmaxf(m, fabsf(logits[(size_t)(fb + i) * ld + tok[j]]));
  }
  const float m1 = block_tree_fold(m, red, [](float a, float b) { return fmaxf(a, b); }) + 1.0f;  // alignment_prob + (max|p| + 1.0): the offset is formed first, as float32

  // row 0 (Aligner.py:211-213): log_p[0, 0] = log(p + M + 1), -inf elsewhere
  float* prev = rows;
  float* cur = rows + lpad;
  for (int j = tid; j < lpad; j += MAS_THREADS) prev[j] = j == 0 ? log_rn(logits[(size_t)fb * ld + tok[0]] + m1) : -INFINITY;
  __syncthreads();
  // rows 1 .. T-1 (Aligner.py:215-225): one float32 add per cell; ties (>=, also between -inf) go to j - 1
  for (int i = 1; i < T; ++i) {
    const float* lr = logits + (size_t)(fb + i) * ld;
    for (int j0 = 0; j0 < W * 64; j0 += MAS_THREADS) {
      const int j = j0 + tid;  // all 64 lanes of a wavefront take part in the ballot; a wavefront covers one bit word
      bool take = false;
      if (j < L) {
        const float stay = prev[j];
        take = j > 0 && prev[j - 1] >= stay;
        cur[j] = log_rn(lr[tok[j]] + m1) + (take ? prev[j - 1] : stay);
      }
      const unsigned long long mask = __ballot(take);
      if (j < W * 64 && (tid & 63) == 0) bits[(size_t)i * W + (j >> 6)] = mask;
    }
    __syncthreads();
    float* t = prev;
    prev = cur;
    cur = t;
  }
  if (off >= 0) __threadfence_block();

  if (tid == 0) {
    // backtrack (Aligner.py:227-233) counting frames per token (DurationCalculator: argmax of each frame row).  The reference sets
    // opt[0, 0] = 1 after the walk and argmax takes the first 1, so frame 0 always counts for token 0.
    int* dur = out;  // the non-boundary durations are built in the first L slots of the output, then spread
    for (int j = 0; j < L; ++j) dur[j] = 0;
    int curr = L - 1;
    for (int i = T - 1; i >= 1; --i) {
      dur[curr] += 1;
      curr -= (int)((bits[(size_t)i * W + (curr >> 6)] >> (curr & 63)) & 1ull);
    }
    dur[0] += 1;
    // zeros at the word boundaries of the full text (UtteranceCloner.py:99-104), filled from the back so no value is overwritten
    // before it is moved (L <= Lf; bit 0 of flags = word boundary)
    int src = L - 1;
    for (int k = Lf - 1; k >= 0; --k) out[k] = (fl[k] & 1) ? 0 : out[src--];
    // repeated identical phonemes: 3/5 - 2/5 of their sum, sequentially (UtteranceCloner.py:117-131; bit 1 of flags = the feature
    // vector equals the previous one).  int((total / 5) * 3) in float32, truncated.
    for (int k = 1; k < Lf; ++k) {
      if (fl[k] & 2) {
        const int total = out[k - 1] + out[k];
        const int n1 = (int)(((float)total / 5.0f) * 3.0f);
        out[k - 1] = n1;
        out[k] = total - n1;
      }
    }
  }
}

int mas_durations(const float* logits, int ld, const int* frame_begin, const int* n_frames, const int* ids, const int* id_begin, const int* n_ids,
                  const int* flags, const int* full_begin, const int* n_full, const long long* scratch_off, unsigned long long* scratch, int batch,
                  int max_ids, int lds_words, int* durations, hipStream_t st) {
  TTS_CHECK_ARG(logits && frame_begin && n_frames && ids && id_begin && n_ids && flags && full_begin && n_full && scratch_off && durations,
                "mas_durations: null pointer");
  TTS_CHECK_ARG(max_ids > 0 && max_ids <= 8192 && lds_words >= 0 && batch >= 0, "mas_durations: max tokens %d (1 .. 8192), lds words %d",
                max_ids, lds_words);
  const int lpad = (max_ids + 63) / 64 * 64;
  const size_t lds = (size_t)2 * lpad * sizeof(float) + (size_t)lds_words * 8;
  TTS_CHECK_ARG(lds + 2048 <= 160 * 1024, "mas_durations: %zu bytes of LDS requested", lds);  // + the static reduction buffer
  if (batch == 0) return TTS_OK;
  hipLaunchKernelGGL(mas_durations_kernel, dim3(batch), dim3(MAS_THREADS), lds, st, logits, ld, frame_begin, n_frames, ids, id_begin, n_ids, flags,
                     full_begin, n_full, scratch_off, scratch, lpad, lds_words, durations);
  return launch_status("mas_durations");
}

// ---- frame energy: sqrt(max(sum_f re^2 + im^2, 1e-10)) over a spectrum stored as [re | im] (EnergyCalculator.py:68-71) -----------
__global__ __launch_bounds__(256) void frame_energy_kernel(const float* __restrict__ x, int ldx, int bins, float* __restrict__ y, int rows) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* xr = x + (size_t)r * ldx;
  float s = 0.0f;
  for (int c = lane; c < bins; c += 64) {
    const float re = xr[c], im = xr[bins + c];
    s += re * re + im * im;
  }
  s = wave_sum(s);
  if (lane == 0) y[r] = sqrtf(fmaxf(s, 1.0e-10f));
}

int frame_energy(const float* x, int ldx, int bins, float* y, int rows, hipStream_t st) {
  TTS_CHECK_ARG(x && y && rows >= 0 && bins > 0 && ldx >= 2 * bins, "frame_energy: bad arguments");
  if (rows == 0) return TTS_OK;
  hipLaunchKernelGGL(frame_energy_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, ldx, bins, y, rows);
  return launch_status("frame_energy");
}

// ---- token averages over the durations, then division by the mean of the nonzero entries ----------------------------------------
// mode 0 (energy, EnergyCalculator._average_by_duration + norm_by_average): mean of every frame of the token; mode 1 (pitch,
// PitchCalculator._average_by_duration): mean of the frames > 0.  keep[k] == 0 zeroes token k (not a phoneme / not voiced).
constexpr int AVG_THREADS = 256;

__global__ __launch_bounds__(AVG_THREADS) void token_average_kernel(const float* __restrict__ x, const int* __restrict__ frame_begin,
                                                                    const int* __restrict__ n_frames, const int* __restrict__ durations,
                                                                    const int* __restrict__ keep, const int* __restrict__ full_begin,
                                                                    const int* __restrict__ n_full, int mode, float* __restrict__ out) {
  extern __shared__ int cum[];  // [max_full + 1]
  __shared__ float rs[AVG_THREADS];
  __shared__ int rc[AVG_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = n_frames[b], Lf = n_full[b], f0 = full_begin[b];
  const float* xr = x + frame_begin[b];
  if (tid == 0) {
    int c = 0;
    cum[0] = 0;
    for (int k = 0; k < Lf; ++k) {
      c += max(durations[f0 + k], 0);
      cum[k + 1] = c;
    }
  }
  __syncthreads();
  float s_nz = 0.0f;
  int n_nz = 0;
  for (int k = tid; k < Lf; k += AVG_THREADS) {
    const int a = min(cum[k], T), e = min(cum[k + 1], T);
    float s = 0.0f;
    int n = 0;
    for (int t = a; t < e; ++t) {
      const float v = xr[t];
      if (mode == 0 || v > 0.0f) {
        s += v;
        ++n;
      }
    }
    const float avg = (n > 0 && keep[f0 + k] != 0) ? s / (float)n : 0.0f;
    out[f0 + k] = avg;
    if (avg != 0.0f) {
      s_nz += avg;
      ++n_nz;
    }
  }
  rs[tid] = s_nz;
  rc[tid] = n_nz;
  __syncthreads();
  for (int o = AVG_THREADS / 2; o > 0; o >>= 1) {  // fixed-order tree: deterministic
    if (tid < o) {
      rs[tid] += rs[tid + o];
      rc[tid] += rc[tid + o];
    }
    __syncthreads();
  }
  const float mean = rs[0] / (float)rc[0];  // no nonzero token: NaN, as the reference's mean of an empty selection
  for (int k = tid; k < Lf; k += AVG_THREADS) out[f0 + k] = out[f0 + k] / mean;
}

int token_average(const float* x, const int* frame_begin, const int* n_frames, const int* durations, const int* keep, const int* full_begin,
                  const int* n_full, int batch, int max_full, int mode, float* out, hipStream_t st) {
  TTS_CHECK_ARG(x && frame_begin && n_frames && durations && keep && full_begin && n_full && out, "token_average: null pointer");
  TTS_CHECK_ARG(max_full > 0 && max_full <= 16384 && (mode == 0 || mode == 1) && batch >= 0, "token_average: max tokens %d, mode %d",
                max_full, mode);
  if (batch == 0) return TTS_OK;
  hipLaunchKernelGGL(token_average_kernel, dim3(batch), dim3(AVG_THREADS), (size_t)(max_full + 1) * sizeof(int), st, x, frame_begin, n_frames,
                     durations, keep, full_begin, n_full, mode, out);
  return launch_status("token_average");
}

}  // namespace tts

extern "C" {
int tts_relu_affine(const float* x, int32_t ldx, float* y, int32_t ldy, int32_t rows, int32_t c, const float* scale, const float* shift,
                    tts_stream_t stream) {
  return tts::relu_affine(x, ldx, y, ldy, rows, c, scale, shift, reinterpret_cast<hipStream_t>(stream));
}
int tts_lstm_recurrence(const float* xproj, int32_t ldx, const float* w_hh_blk, const float* h_in, const float* c_in, float* h_out, float* c_out,
                        float* y, int32_t ldy, const int32_t* seq_begin, const int32_t* seq_len, int32_t batch, int32_t hidden, int32_t step,
                        tts_stream_t stream) {
  return tts::lstm_step(xproj, ldx, w_hh_blk, h_in, c_in, h_out, c_out, y, ldy, seq_begin, seq_len, batch, hidden, step,
                        reinterpret_cast<hipStream_t>(stream));
}
int tts_mas_durations(const float* logits, int32_t ld, const int32_t* frame_begin, const int32_t* n_frames, const int32_t* ids,
                      const int32_t* id_begin, const int32_t* n_ids, const int32_t* flags, const int32_t* full_begin, const int32_t* n_full,
                      const int64_t* scratch_off, uint64_t* scratch, int32_t batch, int32_t max_ids, int32_t lds_words, int32_t* durations,
                      tts_stream_t stream) {
  return tts::mas_durations(logits, ld, frame_begin, n_frames, ids, id_begin, n_ids, flags, full_begin, n_full,
                            reinterpret_cast<const long long*>(scratch_off), reinterpret_cast<unsigned long long*>(scratch), batch, max_ids,
                            lds_words, durations, reinterpret_cast<hipStream_t>(stream));
}
int tts_frame_energy(const float* x, int32_t ldx, int32_t bins, float* y, int32_t rows, tts_stream_t stream) {
  return tts::frame_energy(x, ldx, bins, y, rows, reinterpret_cast<hipStream_t>(stream));
}
int tts_token_average(const float* x, const int32_t* frame_begin, const int32_t* n_frames, const int32_t* durations, const int32_t* keep,
                      const int32_t* full_begin, const int32_t* n_full, int32_t batch, int32_t max_full, int32_t mode, float* out,
                      tts_stream_t stream) {
  return tts::token_average(x, frame_begin, n_frames, durations, keep, full_begin, n_full, batch, max_full, mode, out,
                            reinterpret_cast<hipStream_t>(stream));
}
}
