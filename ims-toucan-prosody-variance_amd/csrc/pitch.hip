// Pitch tracking for the prosody cloner: the autocorrelation method of Boersma (1993) with Praat's documented defaults, as the
// reference calls it (Preprocessing/PitchCalculator.py:64-67: time step 256/16000 s, floor 40 Hz, ceiling 600 Hz).  Written from the
// published algorithm (DESIGN.md section 12 holds the definition); PARITY UNPINNED - Praat is not available to compare against.
//
//   tts_wave_stats        per utterance: mean, and peak after mean removal
//   tts_pitch_candidates  per frame: windowed segment -> normalised autocorrelation r[0 .. 599] -> up to 15 candidates
//   tts_pitch_path        per utterance: Viterbi over the candidates, back-track, f0 per frame
//
// Batch independence: every kernel computes an utterance (a frame) in an order that depends on that utterance alone; the
// reductions are fixed trees, there are no atomics and no workgroup waits on another one.
#include "common.h"
#include "../../include/toucan_pitch.h"

namespace tts {

constexpr int P_SR = 16000, P_HOP = 256;
constexpr int P_NPER = 400;          // floor(16000 / 40): one period of the floor
constexpr int P_HPER = 201;          // nper / 2 + 1
constexpr int P_HW = 599;            // floor(0.075 * 16000) / 2 - 1
constexpr int P_NW = 2 * P_HW;       // 1198 samples: 3 periods of the floor
constexpr int P_MAXLAG = 401;        // nw / 3 + 2
constexpr int P_BIX = 599;           // nw / 2: r[-599 .. 599] feeds the interpolation
constexpr int P_NR = TTS_PITCH_LAGS; // 600 values r[0 .. 599]
constexpr int P_MIN_SAMPLES = 1200;
constexpr int P_CAND = TTS_PITCH_CANDIDATES;  // 15: one unvoiced, at most 14 voiced
constexpr int P_THREADS = 256;
constexpr double P_CEILING = 600.0, P_FLOOR = 40.0;
constexpr double P_SILENCE = 0.03, P_VOICING = 0.45, P_OCTAVE = 0.01, P_JUMP = 0.35, P_VUV = 0.14;
constexpr double P_PI = 3.14159265358979323846;
constexpr double P_GOLD = 0.61803398874989484820;  // (sqrt(5) - 1) / 2
constexpr int P_GOLD_STEPS = 45;                   // 2 * P_GOLD^45 < 1e-9

// the workgroup's 256 values in the LDS tree's order (wave_ops.h block_tree_fold: not the butterfly's)
static_assert(P_THREADS == 256, "block_tree_fold is a tree over 256 threads");
__device__ inline double tree_sum(double v, double* red) {
  return block_tree_fold(v, red, [](double a, double b) { return a + b; });
}
__device__ inline float tree_maxf(float v, float* red) {
  return block_tree_fold(v, red, [](float a, float b) { return fmaxf(a, b); });
}

// ---- mean and peak of every utterance, one workgroup each ------------------------------------------------------------------------
__global__ __launch_bounds__(P_THREADS) void wave_stats_kernel(const float* __restrict__ wave, const int* __restrict__ wave_begin,
                                                               const int* __restrict__ n_samples, float* __restrict__ stats) {
  __shared__ double red[P_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x, n = n_samples[b];
  const float* x = wave + wave_begin[b];
  double s = 0.0;
  for (int i = tid; i < n; i += P_THREADS) s += (double)x[i];
  const float mean = n > 0 ? (float)(tree_sum(s, red) / (double)n) : 0.0f;
  float m = 0.0f;
  for (int i = tid; i < n; i += P_THREADS) m = fmaxf(m, fabsf(x[i] - mean));  // the subtraction the candidates kernel repeats
  m = tree_maxf(m, reinterpret_cast<float*>(red));
  if (tid == 0) {
    stats[2 * b] = mean;
    stats[2 * b + 1] = m;
  }
}

int wave_stats(const float* wave, const int* wave_begin, const int* n_samples, int batch, float* stats, hipStream_t st) {
  TTS_CHECK_ARG(wave && wave_begin && n_samples && stats && batch >= 0, "wave_stats: bad arguments");
  if (batch == 0) return TTS_OK;
  hipLaunchKernelGGL(wave_stats_kernel, dim3(batch), dim3(P_THREADS), 0, st, wave, wave_begin, n_samples, stats);
  return launch_status("wave_stats");
}

// ---- candidates of one frame ---------------------------------------------------------------------------------------------------
// S_D(x): Hann-windowed sinc interpolation of r[-599 .. 599] (r[-k] = r[k]) over at most `depth` samples either side of x, by one
// whole wavefront: lane-strided terms, then wave_sum (wave_ops.h).  sin(pi (x - m)) is (-1)^k sin(pi frac) for the k-th sample on
// either side, so one sine serves every term.  Every lane returns the sum.
__device__ inline double sinc_wave(const double* r, double x, int depth) {
  const int lane = threadIdx.x & 63;
  const double fl = floor(x);
  const int l = (int)fl;
  if (x == fl) return r[min(abs(l), P_BIX)];
  const int dep = min(min(depth, l + P_BIX + 1), P_BIX - l);
  const double dl = x - fl, dr = (fl + 1.0) - x;
  const double sl = sin(P_PI * dl), sr = sin(P_PI * dr);
  const double wl = x - (double)(l + 1 - dep) + 1.0, wr = (double)(l + dep) - x + 1.0;
  double sum = 0.0;
  for (int t = lane; t < 2 * dep; t += 64) {
    const bool left = t < dep;
    const int k = left ? t : t - dep;
    const int m = left ? l - k : l + 1 + k;
    const double a = P_PI * ((left ? dl : dr) + (double)k);
    const double s = (k & 1) ? -(left ? sl : sr) : (left ? sl : sr);
    sum += r[abs(m)] * s / a * (0.5 + 0.5 * cos(a / (left ? wl : wr)));
  }
  return wave_sum(sum);
}

// Ordered compaction by one wavefront: list[] <- the indices i in [lo, hi) with pred(i), ascending, at most `cap` of them; every
// lane returns their number.
template <typename Pred>
__device__ inline int compact_wave0(int lo, int hi, int cap, int* list, Pred pred) {
  const int lane = threadIdx.x & 63;
  int count = 0;
  for (int base = lo; base < hi; base += 64) {
    const int i = base + lane;
    const bool take = i < hi && pred(i);
    const unsigned long long mask = __ballot(take);
    const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));
    if (take && pos < cap) list[pos] = i;
    count += __popcll(mask);
  }
  return min(count, cap);
}

constexpr int AC_LAGS = 8;                      // lags a thread keeps in registers
constexpr int AC_GROUPS = P_NR / AC_LAGS;       // 75 lag groups
constexpr int AC_PARTS = 3;                     // slices of the sample range; 75 * 3 = 225 of the 256 threads work
constexpr int AC_SPAN = 400;                    // samples per slice (a multiple of 8)
constexpr int SEG_PAD = AC_PARTS * AC_SPAN + P_NR + AC_LAGS;  // 1808: the segment, then zeros up to the last sample any product reads
constexpr int MAX_RAW = 200;                    // local maxima among the lags 2 .. 400: at most every second one

__global__ __launch_bounds__(P_THREADS) void pitch_candidates_kernel(const float* __restrict__ wave, const int* __restrict__ wave_begin,
                                                                     const int* __restrict__ n_samples, const float* __restrict__ stats,
                                                                     const int* __restrict__ frame_begin, const int* __restrict__ n_frames,
                                                                     const float* __restrict__ win, const double* __restrict__ wr,
                                                                     float* __restrict__ freq, float* __restrict__ strength,
                                                                     int* __restrict__ n_cand, float* __restrict__ r_out) {
  __shared__ __align__(16) float seg[SEG_PAD];
  __shared__ float part[AC_PARTS][P_NR];
  __shared__ double r[P_NR];
  __shared__ double red[P_THREADS];
  __shared__ int raw[MAX_RAW], kept[P_CAND];
  __shared__ double score[MAX_RAW];
  __shared__ unsigned char keep_flag[MAX_RAW];
  __shared__ int n_raw, n_kept;
  const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nfr = n_frames[b];
  if (f >= nfr) return;
  const int n = n_samples[b];
  const size_t row = (size_t)frame_begin[b] + f;
  float* fq = freq + row * P_CAND;
  float* sg = strength + row * P_CAND;
  // low sample of the frame centre: floor(t / dx - 0.5) = floor((n - 256 nfr + 255) / 2) + 256 f, in integers
  const long long left = (((long long)n - (long long)P_HOP * nfr + P_HOP - 1) >> 1) + (long long)P_HOP * f;
  const long long first = left + 1 - P_HW;  // sample of seg[0]
  if (n < P_MIN_SAMPLES || first < 0 || first + P_NW > n) {  // n_frames does not belong to n_samples: report, read nothing
    if (tid < P_CAND) fq[tid] = sg[tid] = 0.0f;
    if (tid == 0) n_cand[row] = -1;
    return;
  }
  const float* x = wave + wave_begin[b] + first;
  const float gmean = stats[2 * b], gpeak = stats[2 * b + 1];

  // the mean-free samples, their local mean over right - nper .. left + nper (seg index 199 .. 998), the windowed segment
  double s = 0.0;
  for (int j = tid; j < SEG_PAD; j += P_THREADS) {
    const float v = j < P_NW ? x[j] - gmean : 0.0f;
    seg[j] = v;
    if (j >= P_HW - P_NPER && j < P_HW + P_NPER) s += (double)v;
  }
  const float lmean = (float)(tree_sum(s, red) / (double)(2 * P_NPER));
  float lp = 0.0f;
  for (int j = tid; j < P_NW; j += P_THREADS) {
    const float v = (seg[j] - lmean) * win[j];
    seg[j] = v;
    if (j >= P_HW - P_HPER && j < P_HW + P_HPER) lp = fmaxf(lp, fabsf(v));
  }
  lp = tree_maxf(lp, reinterpret_cast<float*>(red));  // its barriers also publish seg
  const float intensity = gpeak > 0.0f ? fminf(1.0f, lp / gpeak) : 0.0f;

  // ac[k] = sum_j seg[j] seg[j + k]: thread (slice p, group g) keeps the lags 8g .. 8g + 7 in registers over the samples of its
  // slice, in ascending j; a loaded sample serves 8 products and the sliding window of 15 neighbours is reloaded half at a time
  if (tid < AC_GROUPS * AC_PARTS) {
    const int p = tid / AC_GROUPS, g = tid - p * AC_GROUPS, k0 = g * AC_LAGS;
    float acc[AC_LAGS];
#pragma unroll
    for (int q = 0; q < AC_LAGS; ++q) acc[q] = 0.0f;
    const float* a = seg + p * AC_SPAN;
    const float* w = a + k0;
    f32x4 w0 = *reinterpret_cast<const f32x4*>(w), w1 = *reinterpret_cast<const f32x4*>(w + 4);
    for (int j = 0; j < AC_SPAN; j += 8) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + j), a1 = *reinterpret_cast<const f32x4*>(a + j + 4);
      const f32x4 w2 = *reinterpret_cast<const f32x4*>(w + j + 8), w3 = *reinterpret_cast<const f32x4*>(w + j + 12);
      const float av[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      const float wn[16] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3], w3[0], w3[1], w3[2], w3[3]};
#pragma unroll
      for (int jj = 0; jj < 8; ++jj)
#pragma unroll
        for (int q = 0; q < AC_LAGS; ++q) acc[q] = fmaf(av[jj], wn[jj + q], acc[q]);
      w0 = w2;
      w1 = w3;
    }
#pragma unroll
    for (int q = 0; q < AC_LAGS; ++q) part[p][k0 + q] = acc[q];
  }
  __syncthreads();
  const float ac0 = (part[0][0] + part[1][0]) + part[2][0];
  for (int k = tid; k < P_NR; k += P_THREADS) {
    const float ac = (part[0][k] + part[1][k]) + part[2][k];
    const double v = k == 0 ? 1.0 : (ac0 > 0.0f ? (double)ac / ((double)ac0 * wr[k]) : 0.0);
    r[k] = v;
    if (r_out) r_out[row * P_NR + k] = (float)v;
  }
  __syncthreads();

  // local maxima above half the voicing threshold among the lags 2 .. 400, ascending
  if (wv == 0) {
    const double half = 0.5 * P_VOICING;
    const int c = ac0 > 0.0f ? compact_wave0(2, min(P_MAXLAG, P_BIX), MAX_RAW, raw,
                                             [&](int i) { return r[i] > half && r[i] > r[i - 1] && r[i] >= r[i + 1]; })
                             : 0;
    if (lane == 0) n_raw = c;
  }
  __syncthreads();
  const int nr = n_raw;
  // first strength at the parabola's vertex, S30; the pruning score is strength - octave cost * log2(floor / f)
  for (int q = wv; q < nr; q += P_THREADS / 64) {
    const int i = raw[q];
    const double c = r[i], lo = r[i - 1], hi = r[i + 1];
    const double xv = (double)i + 0.5 * (hi - lo) / (2.0 * c - lo - hi);
    double sv = sinc_wave(r, xv, 30);
    if (sv > 1.0) sv = 1.0 / sv;
    if (lane == 0) score[q] = sv - P_OCTAVE * log2(P_FLOOR / ((double)P_SR / xv));
  }
  __syncthreads();
  // more than 14: keep the 14 best scores (ties: the smaller lag); the survivors stay in lag order
  for (int q = tid; q < nr; q += P_THREADS) {
    int rank = 0;
    const double sq = score[q];
    for (int o = 0; o < nr; ++o) rank += (score[o] > sq || (score[o] == sq && o < q)) ? 1 : 0;
    keep_flag[q] = rank < P_CAND - 1;
  }
  __syncthreads();
  if (wv == 0) {
    const int c = compact_wave0(0, nr, P_CAND - 1, kept, [&](int q) { return keep_flag[q] != 0; });
    if (lane == 0) n_kept = c;
  }
  __syncthreads();
  const int nk = n_kept;
  // refinement: maximise S70 over [i - 1, i + 1] by golden section, one wavefront per candidate
  for (int q = wv; q < nk; q += P_THREADS / 64) {
    const int i = raw[kept[q]];
    double a = (double)(i - 1), bb = (double)(i + 1);
    double c = bb - P_GOLD * (bb - a), d = a + P_GOLD * (bb - a);
    double fc = sinc_wave(r, c, 70), fd = sinc_wave(r, d, 70);
    for (int it = 0; it < P_GOLD_STEPS; ++it) {
      if (fc >= fd) {  // the maximum lies in [a, d]
        bb = d;
        fd = fc;
        c = bb - P_GOLD * (bb - a);
        d = a + P_GOLD * (bb - a);
        fc = sinc_wave(r, c, 70);
      } else {  // in [c, b]
        a = c;
        fc = fd;
        c = bb - P_GOLD * (bb - a);
        d = a + P_GOLD * (bb - a);
        fd = sinc_wave(r, d, 70);
      }
    }
    const double xm = 0.5 * (a + bb);
    double sm = sinc_wave(r, xm, 70);
    if (sm > 1.0) sm = 1.0 / sm;
    if (lane == 0) {
      fq[1 + q] = (float)((double)P_SR / xm);
      sg[1 + q] = (float)sm;
    }
  }
  if (tid == 0) {
    fq[0] = 0.0f;
    sg[0] = (float)(P_VOICING + fmax(0.0, 2.0 - (double)intensity / (P_SILENCE / (1.0 + P_VOICING))));
    n_cand[row] = 1 + nk;
  }
  if (tid > nk && tid < P_CAND) fq[tid] = sg[tid] = 0.0f;
}

int pitch_candidates(const float* wave, const int* wave_begin, const int* n_samples, const float* stats, const int* frame_begin,
                     const int* n_frames, int batch, int max_frames, const float* win, const double* wr, float* freq, float* strength,
                     int* n_cand, float* r_out, hipStream_t st) {
  TTS_CHECK_ARG(wave && wave_begin && n_samples && stats && frame_begin && n_frames && win && wr && freq && strength && n_cand,
                "pitch_candidates: null pointer");
  TTS_CHECK_ARG(batch >= 0 && batch <= 65535 && max_frames >= 0, "pitch_candidates: batch %d (<= 65535), max frames %d", batch, max_frames);
  if (batch == 0 || max_frames == 0) return TTS_OK;
  hipLaunchKernelGGL(pitch_candidates_kernel, dim3(max_frames, batch), dim3(P_THREADS), 0, st, wave, wave_begin, n_samples, stats, frame_begin,
                     n_frames, win, wr, freq, strength, n_cand, r_out);
  return launch_status("pitch_candidates");
}

// ---- the path: Viterbi over the candidates of an utterance, one workgroup each -------------------------------------------------
// Thread (c, p) = (tid / 16, tid % 16) holds the transition from candidate p of frame t - 1 to candidate c of frame t; the 16 lanes
// of a candidate reduce to the first maximum by wave_arg_max (wave_ops.h).  Per candidate of a frame, info = (log2 f or -1 when voiceless,
// local value); the first 16 threads prepare frame t + 1 while the transitions of frame t are taken.  Back-pointers: one byte per
// candidate, 16 per frame (byte 15 later holds the chosen candidate), in LDS or in the caller's scratch.
constexpr int PATH_ROW = 16;

struct CandInfo {
  double lf;     // log2(frequency); < 0 marks a voiceless candidate (frequency 0 or above the ceiling)
  double local;  // unvoiced: its strength; above the ceiling: 0; else strength - octave cost * log2(ceiling / f)
};

__device__ inline CandInfo cand_info(float f, float s, bool present) {
  CandInfo ci;
  if (!present) {  // past the frame's candidates: never chosen
    ci.lf = -1.0;
    ci.local = -INFINITY;
  } else if (f == 0.0f) {
    ci.lf = -1.0;
    ci.local = (double)s;
  } else if ((double)f > P_CEILING) {
    ci.lf = -1.0;
    ci.local = 0.0;
  } else {
    ci.lf = log2((double)f);  // f >= 16000 / 401: positive
    ci.local = (double)s - P_OCTAVE * log2(P_CEILING / (double)f);
  }
  return ci;
}

__global__ __launch_bounds__(P_THREADS) void pitch_path_kernel(const float* __restrict__ freq, const float* __restrict__ strength,
                                                               const int* __restrict__ n_cand, const int* __restrict__ frame_begin,
                                                               const int* __restrict__ n_frames, const long long* __restrict__ scratch_off,
                                                               unsigned char* __restrict__ scratch, int lds_frames, float* __restrict__ f0) {
  extern __shared__ __align__(16) unsigned char lds_bp[];
  __shared__ CandInfo info[3][PATH_ROW];
  __shared__ double delta[2][PATH_ROW];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, c = tid >> 4, p = tid & 15;
  const int T = n_frames[b];
  const size_t r0 = (size_t)frame_begin[b];
  const float* fq = freq + r0 * P_CAND;
  const float* sg = strength + r0 * P_CAND;
  const int* nc = n_cand + r0;
  float* out = f0 + r0;
  const long long off = scratch_off[b];
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int t = tid; t < T; t += P_THREADS)
    if (nc[t] < 1 || nc[t] > P_CAND) bad = 1;
  __syncthreads();
  if (T <= 0) return;
  if (bad || (off < 0 && T > lds_frames)) {  // a frame without candidates, or no room for the back-pointers: report
    for (int t = tid; t < T; t += P_THREADS) out[t] = -1.0f;
    return;
  }
  unsigned char* bp = off < 0 ? lds_bp : scratch + off;
  const double corr = P_OCTAVE / ((double)P_HOP / (double)P_SR);

  // the first 16 threads: candidate tid of frame t, loaded one iteration before its info is formed
  const bool loader = tid < PATH_ROW;
  auto present = [&](int t) { return loader && t < T && tid < nc[t]; };
  auto load_f = [&](int t) { return present(t) ? fq[(size_t)t * P_CAND + tid] : 0.0f; };
  auto load_s = [&](int t) { return present(t) ? sg[(size_t)t * P_CAND + tid] : 0.0f; };
  if (loader) {
    info[0][tid] = cand_info(load_f(0), load_s(0), present(0));
    delta[0][tid] = info[0][tid].local;
    info[1][tid] = cand_info(load_f(1), load_s(1), present(1));
  }
  bool nin = present(2);
  float nf = load_f(2), ns = load_s(2);
  __syncthreads();
  for (int t = 1; t < T; ++t) {
    const int cur = t & 1, prev = cur ^ 1;
    if (loader) {
      info[(t + 1) % 3][tid] = cand_info(nf, ns, nin);
      nin = present(t + 2);
      nf = load_f(t + 2);
      ns = load_s(t + 2);
    }
    const CandInfo ip = info[(t - 1) % 3][p], ic = info[t % 3][c];
    const bool up = ip.lf < 0.0, uc = ic.lf < 0.0;
    const double cost = (up && uc) ? 0.0 : (up != uc) ? P_VUV * corr : P_JUMP * corr * fabs(ip.lf - ic.lf);
    double val = delta[prev][p] - cost;  // -inf from a candidate that is not there
    int idx = p;
    wave_arg_max<16>(val, idx);  // the first maximum of the 16 lanes
    if (p == 0) {
      delta[cur][c] = val + ic.local;
      bp[(size_t)t * PATH_ROW + c] = (unsigned char)idx;
    }
    if (off >= 0) __threadfence_block();
    __syncthreads();
  }
  if (tid == 0) {
    const int last = (T - 1) & 1;
    int best = 0;
    for (int k = 1; k < nc[T - 1]; ++k)
      if (delta[last][k] > delta[last][best]) best = k;
    for (int t = T - 1; t >= 0; --t) {  // back-track; byte 15 of a frame's row takes the chosen candidate
      const int next = t > 0 ? bp[(size_t)t * PATH_ROW + best] : 0;
      bp[(size_t)t * PATH_ROW + 15] = (unsigned char)best;
      best = next;
    }
  }
  if (off >= 0) __threadfence_block();
  __syncthreads();
  for (int t = tid; t < T; t += P_THREADS) {
    const float f = fq[(size_t)t * P_CAND + bp[(size_t)t * PATH_ROW + 15]];
    out[t] = (f == 0.0f || (double)f > P_CEILING) ? 0.0f : f;
  }
}

int pitch_path(const float* freq, const float* strength, const int* n_cand, const int* frame_begin, const int* n_frames,
               const long long* scratch_off, unsigned char* scratch, int batch, int lds_frames, float* f0, hipStream_t st) {
  TTS_CHECK_ARG(freq && strength && n_cand && frame_begin && n_frames && scratch_off && f0, "pitch_path: null pointer");
  TTS_CHECK_ARG(batch >= 0 && lds_frames >= 0 && lds_frames <= TTS_PITCH_PATH_LDS_FRAMES, "pitch_path: batch %d, lds frames %d (<= %d)", batch,
                lds_frames, TTS_PITCH_PATH_LDS_FRAMES);
  if (batch == 0) return TTS_OK;
  hipLaunchKernelGGL(pitch_path_kernel, dim3(batch), dim3(P_THREADS), (size_t)lds_frames * PATH_ROW, st, freq, strength, n_cand, frame_begin,
                     n_frames, scratch_off, scratch, lds_frames, f0);
  return launch_status("pitch_path");
}

}  // namespace tts

extern "C" {
int tts_wave_stats(const float* wave, const int32_t* wave_begin, const int32_t* n_samples, int32_t batch, float* stats, tts_stream_t stream) {
  return tts::wave_stats(wave, wave_begin, n_samples, batch, stats, reinterpret_cast<hipStream_t>(stream));
}
int tts_pitch_candidates(const float* wave, const int32_t* wave_begin, const int32_t* n_samples, const float* stats, const int32_t* frame_begin,
                         const int32_t* n_frames, int32_t batch, int32_t max_frames, const float* win, const double* wr, float* freq,
                         float* strength, int32_t* n_cand, float* r_out, tts_stream_t stream) {
  return tts::pitch_candidates(wave, wave_begin, n_samples, stats, frame_begin, n_frames, batch, max_frames, win, wr, freq, strength, n_cand,
                               r_out, reinterpret_cast<hipStream_t>(stream));
}
int tts_pitch_path(const float* freq, const float* strength, const int32_t* n_cand, const int32_t* frame_begin, const int32_t* n_frames,
                   const int64_t* scratch_off, uint8_t* scratch, int32_t batch, int32_t lds_frames, float* f0, tts_stream_t stream) {
  return tts::pitch_path(freq, strength, n_cand, frame_begin, n_frames, reinterpret_cast<const long long*>(scratch_off), scratch, batch,
                         lds_frames, f0, reinterpret_cast<hipStream_t>(stream));
}
}
