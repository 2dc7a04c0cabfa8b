// Checking synthesised speech without a recording (DESIGN.md section 19 holds the definition):
//
//   tts_ctc_best_path      per utterance: the greedy decode of the aligner's posteriors, runs with their frames and confidences
//   tts_ctc_beam_search    per utterance: CTC prefix beam search without a language model
//   tts_edit_distance      per pair: the Levenshtein alignment of the intended and the decoded phonemes
//   tts_phone_posteriors   per utterance: mean log-posterior, goodness of pronunciation and frame accuracy of every token
//
// Batch independence: one workgroup per utterance, every sum in an order that depends on the utterance alone, no atomics and no
// workgroup waits on another one.
#include "common.h"
#include "pair_sweep.h"
#include "../../include/toucan_pronunciation.h"

namespace tts {

constexpr int P_THREADS = 256;
constexpr int P_BLOCK = TTS_CTC_SCAN_BLOCK;
constexpr int P_MAX_SYMBOLS = TTS_PRON_MAX_SYMBOLS;
static_assert(P_BLOCK == P_THREADS, "one thread per frame of a scan block");

// ---- one frame of posteriors ----------------------------------------------------------------------------------------------------
// argmax over the raw fp32 logits (strict >), then log sum_c exp(x_c - max) in fp64 with c in index order:
// lp[c] = ((double)x_c - mx) - lse, the arithmetic of every kernel here
struct FrameStat {
  int arg;
  double mx, lse;
};

__device__ __forceinline__ FrameStat frame_stat(const float* __restrict__ x, int S) {
  FrameStat f;
  f.arg = 0;
  float best = x[0];
  for (int c = 1; c < S; ++c) {
    const float v = x[c];
    if (v > best) {
      best = v;
      f.arg = c;
    }
  }
  f.mx = (double)best;
  double sum = 0.0;
  for (int c = 0; c < S; ++c) sum += exp((double)x[c] - f.mx);
  f.lse = log(sum);
  return f;
}

__device__ __forceinline__ double log_add_exp(double a, double b) {
  const double ninf = -__builtin_huge_val();
  if (a == ninf) return b;
  if (b == ninf) return a;
  const double m = a > b ? a : b;
  return m + log1p(exp(-fabs(a - b)));
}

// 1 in every thread if the utterance holds a logit that is not finite (two barriers; flag: one int of LDS)
__device__ __forceinline__ int any_not_finite(const float* __restrict__ X, int ld, int T, int S, int* flag) {
  if (threadIdx.x == 0) *flag = 0;
  __syncthreads();
  int bad = 0;
  for (int t = 0; t < T; ++t)
    for (int c = threadIdx.x; c < S; c += P_THREADS) bad |= !isfinite(X[(size_t)t * ld + c]);
  if (bad) *flag = 1;
  __syncthreads();
  return *flag;
}

// ---- greedy decode --------------------------------------------------------------------------------------------------------------
// Blocks of 256 frames, one thread per frame.  A thread whose frame opens a run walks the block's symbols forwards and sums the
// run's logp in frame order; the run that reaches the block's end is carried (its sum, count and slot) and thread 0 continues it at
// the head of the next block, so the sum's order is that of the frames whatever the block boundaries.  The slot of a run is the
// count carried from the earlier blocks plus an inclusive scan of the openers.
__global__ __launch_bounds__(P_THREADS) void ctc_best_path_kernel(const float* __restrict__ logits, int ld, int S, int blank,
                                                                  const unsigned char* __restrict__ drop, const TtsPronUtt* __restrict__ utts,
                                                                  int* __restrict__ hyp_id, int* __restrict__ hyp_first, int* __restrict__ hyp_last,
                                                                  float* __restrict__ hyp_conf, int* __restrict__ n_hyp) {
  __shared__ int s_sym[P_BLOCK + 1];  // [0]: the last symbol of the block before
  __shared__ float s_lp[P_BLOCK];
  __shared__ int s_scan[P_BLOCK];
  __shared__ int s_flag, c_active, c_sym, c_first, c_idx, c_cnt;
  __shared__ double c_sum;
  const int b = blockIdx.x, tid = threadIdx.x;
  const TtsPronUtt u = utts[b];
  const int T = u.n_frames;
  const float* X = logits + (size_t)u.frame_begin * ld;
  if (any_not_finite(X, ld, T, S, &s_flag)) {
    if (tid == 0) n_hyp[b] = -1;
    return;
  }
  int* o_id = hyp_id + u.frame_begin;
  int* o_first = hyp_first + u.frame_begin;
  int* o_last = hyp_last + u.frame_begin;
  float* o_conf = hyp_conf + u.frame_begin;
  if (tid == 0) {
    s_sym[0] = -1;  // no symbol: frame 0 opens a run unless it is blank
    c_active = 0;
  }
  int count = 0;  // runs opened in the blocks before (the same in every thread)
  for (int base = 0; base < T; base += P_BLOCK) {
    const int nb = min(P_BLOCK, T - base), t = base + tid;
    int sym = -2;
    if (tid < nb) {
      const FrameStat f = frame_stat(X + (size_t)t * ld, S);
      sym = (f.arg == blank || (drop && drop[f.arg])) ? blank : f.arg;
      s_lp[tid] = (float)(((double)X[(size_t)t * ld + f.arg] - f.mx) - f.lse);
    }
    __syncthreads();  // (the block before has read s_sym and s_scan)
    s_sym[tid + 1] = sym;
    __syncthreads();
    const int open = tid < nb && sym != blank && sym != s_sym[tid];
    s_scan[tid] = open;
    __syncthreads();
    for (int o = 1; o < P_BLOCK; o <<= 1) {
      const int v = tid >= o ? s_scan[tid - o] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    const bool more = base + nb < T;
    if (tid == 0 && c_active) {  // the carried run goes on at the head of this block
      int v = 0;
      while (v < nb && s_sym[v + 1] == c_sym) {
        c_sum += (double)s_lp[v];
        ++c_cnt;
        ++v;
      }
      if (!(v == nb && more)) {
        o_id[c_idx] = c_sym;
        o_first[c_idx] = c_first;
        o_last[c_idx] = base + v - 1;
        o_conf[c_idx] = (float)(c_sum / (double)c_cnt);
        c_active = 0;
      }
    }
    __syncthreads();  // (the carried run is settled before a run of this block takes its place)
    if (open) {
      const int idx = count + s_scan[tid] - 1;
      double sum = (double)s_lp[tid];
      int cnt = 1, v = tid + 1;
      while (v < nb && s_sym[v + 1] == sym) {
        sum += (double)s_lp[v];
        ++cnt;
        ++v;
      }
      if (v == nb && more) {
        c_active = 1;
        c_sym = sym;
        c_first = t;
        c_idx = idx;
        c_cnt = cnt;
        c_sum = sum;
      } else {
        o_id[idx] = sym;
        o_first[idx] = t;
        o_last[idx] = base + v - 1;
        o_conf[idx] = (float)(sum / (double)cnt);
      }
    }
    count += s_scan[P_BLOCK - 1];
    __syncthreads();
    if (tid == 0) s_sym[0] = s_sym[nb];
  }
  if (tid == 0) n_hyp[b] = count;
}

// ---- prefix beam search -----------------------------------------------------------------------------------------------------------
// Per block of 256 frames one thread per frame forms (max, log sum exp); then frame after frame: lp[] of the frame, the marks of
// the extend candidates that merge (child[i][c] = j + 1 when live beam j spells beam i's prefix plus c: beam * beam comparisons,
// see extends_to), the stay candidates, and `beam` rounds of selection.  A candidate's total is recomputed from (beam, symbol) wherever it is needed, by
// the one function cand_total; every thread keeps the best of its candidates q = tid, tid + 256, ... that lies behind its last
// pick in the order (total descending, q ascending), a round takes the best of the 256 and only its owner looks for its next one.
constexpr int B_MAX = TTS_BEAM_MAX;

struct BeamSet {
  int node[B_MAX], par[B_MAX], sym[B_MAX], len[B_MAX];  // node: -1 the empty prefix; par: -2 for it
  unsigned long long hash[B_MAX];                        // of the prefix: hash(P + c) = prefix_hash(hash(P), c)
  double pb[B_MAX], pnb[B_MAX], tot[B_MAX];
};

__device__ __forceinline__ unsigned long long prefix_hash(unsigned long long h, int c) {
  return (h ^ (unsigned long long)(c + 1)) * 0x100000001b3ull;
}

// Does live beam j spell beam i's prefix plus j's last symbol?  A node of the history table is made afresh whenever an extend
// candidate is selected, so one prefix can own several nodes: it is pruned while a child of it lives on, and is made again from its
// own parent.  Node numbers therefore only shorten the answer.  The lengths and the hashes must fit (unequal hashes: unequal
// prefixes); then the two chains are walked back symbol by symbol until they meet in one node or at the root, which is exact.
__device__ __forceinline__ bool extends_to(const BeamSet& bs, int i, int j, const int* hist) {
  if (bs.len[j] != bs.len[i] + 1 || bs.hash[j] != prefix_hash(bs.hash[i], bs.sym[j])) return false;
  int a = bs.par[j], b = bs.node[i];
  while (a != b) {
    if (a < 0 || b < 0 || hist[2 * (size_t)a + 1] != hist[2 * (size_t)b + 1]) return false;  // (equal lengths: both reach the root together)
    a = hist[2 * (size_t)a];
    b = hist[2 * (size_t)b];
  }
  return true;
}

struct Cand {
  double tot;
  int q;
};

// the tie rule of wave_arg_max (wave_ops.h), for the serial picks
__device__ __forceinline__ bool cand_before(double ta, int qa, double tb, int qb) { return arg_before<true>(ta, qa, tb, qb); }

// total of candidate q, or -inf if q is no candidate (blank, dropped, merged into a stay candidate, or without probability)
__device__ __forceinline__ double cand_total(int q, int S, int blank, const unsigned char* __restrict__ drop, const BeamSet& bs,
                                             const double* st_tot, const double* lp, const unsigned char* child) {
  const int i = q / (S + 1), r = q - i * (S + 1);
  if (r == 0) return st_tot[i];
  const int c = r - 1;
  if (c == blank || (drop && drop[c]) || child[i * P_MAX_SYMBOLS + c]) return -__builtin_huge_val();
  return (c == bs.sym[i] ? bs.pb[i] : bs.tot[i]) + lp[c];
}

__device__ __forceinline__ Cand best_behind(int n_cand, double thr_t, int thr_q, int S, int blank, const unsigned char* __restrict__ drop,
                                            const BeamSet& bs, const double* st_tot, const double* lp, const unsigned char* child) {
  Cand best = {-__builtin_huge_val(), 0x7fffffff};
  for (int q = threadIdx.x; q < n_cand; q += P_THREADS) {
    const double t = cand_total(q, S, blank, drop, bs, st_tot, lp, child);
    if (t == -__builtin_huge_val()) continue;
    if (!cand_before(thr_t, thr_q, t, q)) continue;  // not behind the last pick
    if (cand_before(t, q, best.tot, best.q)) best = {t, q};
  }
  return best;
}

__global__ __launch_bounds__(P_THREADS) void ctc_beam_kernel(const float* __restrict__ logits, int ld, int S, int blank,
                                                             const unsigned char* __restrict__ drop, const TtsPronUtt* __restrict__ utts, int W,
                                                             int* __restrict__ scratch, int* __restrict__ hyp_id, int* __restrict__ n_hyp,
                                                             double* __restrict__ score) {
  __shared__ double s_lp[P_MAX_SYMBOLS], s_mx[P_BLOCK], s_lse[P_BLOCK];
  __shared__ unsigned char s_child[B_MAX * P_MAX_SYMBOLS];
  __shared__ BeamSet s_beams[2];
  __shared__ double st_pb[B_MAX], st_pnb[B_MAX], st_tot[B_MAX];
  __shared__ double r_tot[P_THREADS / 64];
  __shared__ int r_q[P_THREADS / 64];
  __shared__ int s_flag, s_live;
  __shared__ int s_src[B_MAX];  // the live beam whose extend candidate is joined into this beam's stay candidate, or -1
  const int b = blockIdx.x, tid = threadIdx.x;
  const TtsPronUtt u = utts[b];
  const int T = u.n_frames;
  const float* X = logits + (size_t)u.frame_begin * ld;
  const double ninf = -__builtin_huge_val();
  if (any_not_finite(X, ld, T, S, &s_flag)) {
    if (tid == 0) n_hyp[b] = -1;
    return;
  }
  int* hist = scratch + u.scratch_off;
  for (int e = tid; e < B_MAX * P_MAX_SYMBOLS; e += P_THREADS) s_child[e] = 0;
  if (tid == 0) {
    BeamSet& z = s_beams[0];
    z.node[0] = -1;
    z.par[0] = -2;
    z.sym[0] = -1;
    z.len[0] = 0;
    z.hash[0] = 0xcbf29ce484222325ull;
    z.pb[0] = 0.0;
    z.pnb[0] = ninf;
    z.tot[0] = 0.0;
    s_live = 1;
  }
  int cur = 0;
  for (int base = 0; base < T; base += P_BLOCK) {
    const int nb = min(P_BLOCK, T - base);
    __syncthreads();  // (the frames of the block before have read s_mx / s_lse; the first block: the initial beam is written)
    if (tid < nb) {
      const FrameStat f = frame_stat(X + (size_t)(base + tid) * ld, S);
      s_mx[tid] = f.mx;
      s_lse[tid] = f.lse;
    }
    __syncthreads();
    for (int v = 0; v < nb; ++v) {
      const int t = base + v;
      const BeamSet& bs = s_beams[cur];
      BeamSet& nx = s_beams[cur ^ 1];
      const int n = s_live;
      for (int c = tid; c < S; c += P_THREADS) s_lp[c] = ((double)X[(size_t)t * ld + c] - s_mx[v]) - s_lse[v];
      if (tid < n) s_src[tid] = -1;
      __syncthreads();
      for (int pr = tid; pr < n * n; pr += P_THREADS) {  // (live beams spell different prefixes: at most one i for a j)
        const int i = pr / n, j = pr - i * n;
        if (extends_to(bs, i, j, hist)) {
          s_child[i * P_MAX_SYMBOLS + bs.sym[j]] = (unsigned char)(j + 1);
          s_src[j] = i;
        }
      }
      __syncthreads();
      if (tid < n) {
        const int e = bs.sym[tid];
        const double pb = bs.tot[tid] + s_lp[blank];
        double pnb = e >= 0 ? bs.pnb[tid] + s_lp[e] : ninf;
        const int i = s_src[tid];
        if (i >= 0) pnb = log_add_exp(pnb, (e == bs.sym[i] ? bs.pb[i] : bs.tot[i]) + s_lp[e]);
        st_pb[tid] = pb;
        st_pnb[tid] = pnb;
        st_tot[tid] = log_add_exp(pb, pnb);
      }
      __syncthreads();
      const int n_cand = n * (S + 1);
      Cand mine = best_behind(n_cand, __builtin_huge_val(), -1, S, blank, drop, bs, st_tot, s_lp, s_child);
      int k = 0;
      for (; k < W; ++k) {
        Cand w = mine;
        wave_arg_max(w.tot, w.q);
        if ((tid & 63) == 0) {
          r_tot[tid >> 6] = w.tot;
          r_q[tid >> 6] = w.q;
        }
        __syncthreads();
        w = {r_tot[0], r_q[0]};
#pragma unroll
        for (int g = 1; g < P_THREADS / 64; ++g)
          if (cand_before(r_tot[g], r_q[g], w.tot, w.q)) w = {r_tot[g], r_q[g]};
        if (w.tot == ninf) {  // (the same in every thread) no candidate is left
          __syncthreads();
          break;
        }
        if (tid == 0) {
          const int i = w.q / (S + 1), r = w.q - i * (S + 1);
          if (r == 0) {
            nx.node[k] = bs.node[i];
            nx.par[k] = bs.par[i];
            nx.sym[k] = bs.sym[i];
            nx.len[k] = bs.len[i];
            nx.hash[k] = bs.hash[i];
            nx.pb[k] = st_pb[i];
            nx.pnb[k] = st_pnb[i];
            nx.tot[k] = st_tot[i];
          } else {
            const int node = t * W + k;
            hist[2 * (size_t)node] = bs.node[i];
            hist[2 * (size_t)node + 1] = r - 1;
            nx.node[k] = node;
            nx.par[k] = bs.node[i];
            nx.sym[k] = r - 1;
            nx.len[k] = bs.len[i] + 1;
            nx.hash[k] = prefix_hash(bs.hash[i], r - 1);
            nx.pb[k] = ninf;
            nx.pnb[k] = w.tot;
            nx.tot[k] = w.tot;
          }
        }
        if (mine.q == w.q) mine = best_behind(n_cand, w.tot, w.q, S, blank, drop, bs, st_tot, s_lp, s_child);
        __syncthreads();  // (r_tot / r_q are free for the next round)
      }
      if (tid < n && s_src[tid] >= 0) s_child[s_src[tid] * P_MAX_SYMBOLS + bs.sym[tid]] = 0;
      if (tid == 0) s_live = k;
      cur ^= 1;
      __syncthreads();
    }
  }
  if (tid == 0) {  // (the stay candidate of the best beam is always finite: at least one beam lives)
    const BeamSet& bs = s_beams[cur];
    int node = bs.node[0];
    const int L = bs.len[0];
    int* out = hyp_id + u.frame_begin;
    for (int p = L - 1; p >= 0; --p) {  // a prefix grows by at most one symbol per frame: L <= T
      out[p] = hist[2 * (size_t)node + 1];
      node = hist[2 * (size_t)node];
    }
    n_hyp[b] = L;
    score[b] = bs.tot[0];
  }
}

// ---- edit distance, one workgroup per pair --------------------------------------------------------------------------------------
// The sweep of pair_sweep.h over integer costs, rows (reference tokens) and columns (decoded tokens) counted from 1: D(i, 0) = i,
// D(0, j) = j, a thread keeps its reference token and a cell takes the diagonal plus a mismatch, a deletion (up) plus 1 or an
// insertion (left) plus 1.  Thread 0 walks back and writes both maps as it goes: every token is met exactly once.
constexpr int E_MAX_HYP = TTS_EDIT_MAX_HYP;
static_assert(P_THREADS == SWEEP_THREADS, "the sweep's workgroup");
static_assert(4 * (E_MAX_HYP + 1) + 4 * E_MAX_HYP + 8 * P_THREADS + TTS_EDIT_LDS_BP_BYTES + 64 <= 64 * 1024, "LDS budget without a raised limit");

struct EditCells {
  using value_t = int;
  static constexpr int ORIGIN = 1;
  const int *ref, *hyp;
  int mine;

  __device__ __forceinline__ void band(int i, bool active) { mine = active ? ref[i - 1] : 0; }
  __device__ __forceinline__ int border(int i, int j) const { return j == 0 ? i : j; }  // D(i, 0) = i, D(0, j) = j
  __device__ __forceinline__ void step(int, bool) const {}
  __device__ __forceinline__ int via(unsigned int code, int pred, int j) const { return pred + (code || mine != hyp[j - 1] ? 1 : 0); }
  __device__ __forceinline__ int cell(int, int, int best) const { return best; }
  __device__ __forceinline__ void last(int) const {}
};

__global__ __launch_bounds__(P_THREADS) void edit_distance_kernel(const int* __restrict__ ref_ids, const int* __restrict__ hyp_id,
                                                                  const int* __restrict__ n_hyp, const TtsPronUtt* __restrict__ utts,
                                                                  unsigned char* __restrict__ scratch, int* __restrict__ counts,
                                                                  int* __restrict__ ref_to_hyp, int* __restrict__ hyp_to_ref) {
  extern __shared__ __align__(16) unsigned char e_lds[];
  __shared__ int row[E_MAX_HYP + 1];
  __shared__ int hyp_s[E_MAX_HYP];
  __shared__ int diag[2 * P_THREADS];
  const int p = blockIdx.x, tid = threadIdx.x;
  const TtsPronUtt u = utts[p];
  const int R = u.n_ref, H = n_hyp[p];
  if (H < 0 || H > min(u.n_frames, E_MAX_HYP)) {  // (the same decision in every thread)
    if (tid < 4) counts[4 * (size_t)p + tid] = -1;
    return;
  }
  const int* ref = ref_ids + u.ref_begin;
  const int Wd = (H + 15) >> 4;
  for (int j = tid; j < H; j += P_THREADS) hyp_s[j] = hyp_id[(size_t)u.frame_begin + j];
  __syncthreads();
  EditCells cells = {ref, hyp_s, 0};
  const unsigned int* bp = pair_sweep(cells, R, H, row, diag, u.scratch_off, e_lds, scratch);
  if (tid == 0) {
    int* r2h = ref_to_hyp + u.ref_begin;
    int* h2r = hyp_to_ref + u.frame_begin;
    int i = R, j = H, hits = 0, subs = 0, dels = 0, ins = 0;
    while (i > 0 || j > 0) {
      const unsigned int code = i == 0 ? 2u : j == 0 ? 1u : bp_code<EditCells::ORIGIN>(bp, Wd, i, j);
      if (code == 0) {
        if (ref[i - 1] == hyp_s[j - 1]) ++hits;
        else ++subs;
        r2h[i - 1] = j - 1;
        h2r[j - 1] = i - 1;
        --i;
        --j;
      } else if (code == 1) {
        ++dels;
        r2h[i - 1] = -1;
        --i;
      } else {
        ++ins;
        h2r[j - 1] = -1;
        --j;
      }
    }
    int* c = counts + 4 * (size_t)p;
    c[0] = hits;
    c[1] = subs;
    c[2] = dels;
    c[3] = ins;
  }
}

// ---- posteriors over the forced alignment ---------------------------------------------------------------------------------------
// Tokens in chunks of 256: an inclusive scan of the durations with the sum of the chunks before carried gives every token's first
// frame.  The four wavefronts then take the chunk's tokens in turn; a wavefront forms 64 frames of its token at a time, one lane per
// frame, and every lane adds the 64 values in frame order (read lane by lane), so the sums are those of a loop over the frames.
// What makes the utterance invalid (a negative duration, a token that leaves the frames, a total that is not n_frames) is collected
// in a flag, and the rows are overwritten with NaN at the end.
__global__ __launch_bounds__(P_THREADS) void phone_posteriors_kernel(const float* __restrict__ logits, int ld, int S, const int* __restrict__ durations,
                                                                     const int* __restrict__ token_ids, const TtsPronUtt* __restrict__ utts,
                                                                     float* __restrict__ out) {
  __shared__ long long s_scan[P_THREADS];
  __shared__ int s_first[P_THREADS], s_d[P_THREADS], s_id[P_THREADS];  // s_d: -1 for a token that is not computed
  __shared__ int s_bad;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const TtsPronUtt u = utts[b];
  const int T = u.n_frames, K = u.n_ref;
  const float* X = logits + (size_t)u.frame_begin * ld;
  const int* dur = durations + u.ref_begin;
  const int* ids = token_ids + u.ref_begin;
  float* o = out + (size_t)TTS_PHONE_COLUMNS * u.ref_begin;
  const float nanf_ = __builtin_nanf("");
  if (tid == 0) s_bad = 0;
  long long carried = 0;  // frames of the chunks before (the same in every thread)
  for (int k0 = 0; k0 < K; k0 += P_THREADS) {
    const int k = k0 + tid;
    const int d = k < K ? dur[k] : 0;
    __syncthreads();  // (the wavefronts are through with the chunk before; the first chunk: s_bad is cleared)
    s_scan[tid] = d > 0 ? d : 0;
    __syncthreads();
    for (int off = 1; off < P_THREADS; off <<= 1) {
      const long long v = tid >= off ? s_scan[tid - off] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    const long long first = carried + s_scan[tid] - (d > 0 ? d : 0);
    const bool leaves = k < K && (d < 0 || first + d > T);
    if (leaves) s_bad = 1;
    s_first[tid] = (int)(first < T ? first : T);
    s_d[tid] = (k < K && !leaves) ? d : -1;
    s_id[tid] = k < K ? ids[k] : -1;
    carried += s_scan[P_THREADS - 1];
    __syncthreads();
    const int nk = min(P_THREADS, K - k0);
    for (int j = wave; j < nk; j += P_THREADS / 64) {  // (everything here is the same in the 64 lanes of a wavefront)
      const int dj = s_d[j], id = s_id[j], f0 = s_first[j];
      float* row = o + 4 * (size_t)(k0 + j);
      if (dj < 0) continue;
      if (dj == 0 || id < 0 || id >= S) {
        if (lane < 3) row[lane] = nanf_;
        if (lane == 3) row[3] = (float)dj;
        continue;
      }
      double s_post = 0.0, s_gop = 0.0;
      int hits = 0;
      for (int c = 0; c < dj; c += 64) {
        const int m = min(64, dj - c);
        double v_post = 0.0, v_gop = 0.0;
        int hit = 0;
        if (lane < m) {
          const float* x = X + (size_t)(f0 + c + lane) * ld;
          const FrameStat f = frame_stat(x, S);
          v_post = ((double)x[id] - f.mx) - f.lse;
          v_gop = v_post - (((double)x[f.arg] - f.mx) - f.lse);
          hit = f.arg == id;
        }
        for (int l = 0; l < m; ++l) {
          s_post += __shfl(v_post, l, 64);
          s_gop += __shfl(v_gop, l, 64);
          hits += __shfl(hit, l, 64);
        }
      }
      if (lane == 0) {
        row[0] = (float)(s_post / (double)dj);
        row[1] = (float)(s_gop / (double)dj);
        row[2] = (float)((double)hits / (double)dj);
        row[3] = (float)dj;
      }
    }
  }
  __syncthreads();
  if (s_bad || carried != T)
    for (int e = tid; e < TTS_PHONE_COLUMNS * K; e += P_THREADS) o[e] = nanf_;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// checks the host table, then copies it to the device on the stream
static int upload_utts(const char* what, const TtsPronUtt* host, TtsPronUtt* dev, int n, int rows, long long n_ref_total, int max_ref,
                       hipStream_t st) {
  for (int b = 0; b < n; ++b) {
    const TtsPronUtt& q = host[b];
    TTS_CHECK_ARG(q.n_frames >= 1 && q.frame_begin >= 0 && (long long)q.frame_begin + q.n_frames <= rows,
                  "%s: utterance %d: frames %d + %d lie outside the %d rows (at least one frame)", what, b, q.frame_begin, q.n_frames, rows);
    if (n_ref_total < 0) continue;
    TTS_CHECK_ARG(q.n_ref >= 0 && q.n_ref <= max_ref && q.ref_begin >= 0 && (long long)q.ref_begin + q.n_ref <= n_ref_total,
                  "%s: utterance %d: tokens %d + %d lie outside the %lld given (at most %d per utterance)", what, b, q.ref_begin, q.n_ref,
                  n_ref_total, max_ref);
  }
  const hipError_t e = hipMemcpyAsync(dev, host, (size_t)n * sizeof(TtsPronUtt), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    set_error("%s: copying the utterance table: %s", what, hipGetErrorString(e));
    return TTS_E_LAUNCH;
  }
  return TTS_OK;
}

static int check_logits(const char* what, const float* logits, int rows, int ld, int S, int blank) {
  TTS_CHECK_ARG(logits != nullptr && rows >= 0, "%s: no logits, or %d rows", what, rows);
  TTS_CHECK_ARG(S >= 1 && S <= P_MAX_SYMBOLS && ld >= S, "%s: %d symbols (1 .. %d) in rows of %d", what, S, P_MAX_SYMBOLS, ld);
  TTS_CHECK_ARG(blank >= 0 && blank < S, "%s: blank %d is none of the %d symbols", what, blank, S);
  return TTS_OK;
}

int ctc_best_path(const float* logits, int rows, int ld, int S, int blank, const unsigned char* drop, const TtsPronUtt* host, TtsPronUtt* dev,
                  int n, int* hyp_id, int* hyp_first, int* hyp_last, float* hyp_conf, int* n_hyp, hipStream_t st) {
  TTS_CHECK_ARG(n >= 0, "ctc_best_path: %d utterances", n);
  if (n == 0) return TTS_OK;
  int rc = check_logits("ctc_best_path", logits, rows, ld, S, blank);
  if (rc != TTS_OK) return rc;
  TTS_CHECK_ARG(host && dev && hyp_id && hyp_first && hyp_last && hyp_conf && n_hyp, "ctc_best_path: null pointer");
  rc = upload_utts("ctc_best_path", host, dev, n, rows, -1, 0, st);
  if (rc != TTS_OK) return rc;
  hipLaunchKernelGGL(ctc_best_path_kernel, dim3(n), dim3(P_THREADS), 0, st, logits, ld, S, blank, drop, dev, hyp_id, hyp_first, hyp_last, hyp_conf,
                     n_hyp);
  return launch_status("ctc_best_path");
}

int ctc_beam_search(const float* logits, int rows, int ld, int S, int blank, const unsigned char* drop, const TtsPronUtt* host, TtsPronUtt* dev,
                    int n, int W, int* scratch, long long scratch_words, int* hyp_id, int* n_hyp, double* score, hipStream_t st) {
  TTS_CHECK_ARG(n >= 0, "ctc_beam_search: %d utterances", n);
  TTS_CHECK_ARG(W >= 1 && W <= B_MAX, "ctc_beam_search: a beam of %d (1 .. %d)", W, B_MAX);
  if (n == 0) return TTS_OK;
  int rc = check_logits("ctc_beam_search", logits, rows, ld, S, blank);
  if (rc != TTS_OK) return rc;
  TTS_CHECK_ARG(host && dev && scratch && hyp_id && n_hyp && score, "ctc_beam_search: null pointer");
  for (int b = 0; b < n; ++b) {
    const long long need = 2ll * host[b].n_frames * W;
    TTS_CHECK_ARG(host[b].n_frames <= (1 << 24), "ctc_beam_search: utterance %d: %d frames (at most %d)", b, host[b].n_frames, 1 << 24);
    TTS_CHECK_ARG(host[b].scratch_off >= 0 && host[b].scratch_off + need <= scratch_words,
                  "ctc_beam_search: utterance %d: its history table (%lld words at %lld) lies outside the %lld words of scratch", b, need,
                  (long long)host[b].scratch_off, scratch_words);
  }
  rc = upload_utts("ctc_beam_search", host, dev, n, rows, -1, 0, st);
  if (rc != TTS_OK) return rc;
  hipLaunchKernelGGL(ctc_beam_kernel, dim3(n), dim3(P_THREADS), 0, st, logits, ld, S, blank, drop, dev, W, scratch, hyp_id, n_hyp, score);
  return launch_status("ctc_beam_search");
}

int edit_distance(const int* ref_ids, int n_ref_total, const int* hyp_id, int rows, const int* n_hyp, const TtsPronUtt* host, TtsPronUtt* dev, int n,
                  unsigned char* scratch, long long scratch_bytes, int lds_bp_bytes, int* counts, int* ref_to_hyp, int* hyp_to_ref, hipStream_t st) {
  TTS_CHECK_ARG(n >= 0 && rows >= 0 && n_ref_total >= 0, "edit_distance: %d pairs, %d rows, %d reference tokens", n, rows, n_ref_total);
  if (n == 0) return TTS_OK;
  TTS_CHECK_ARG(ref_ids && hyp_id && n_hyp && host && dev && counts && ref_to_hyp && hyp_to_ref, "edit_distance: null pointer");
  TTS_CHECK_ARG(lds_bp_bytes >= 0 && lds_bp_bytes <= TTS_EDIT_LDS_BP_BYTES && lds_bp_bytes % 16 == 0,
                "edit_distance: %d bytes of LDS for back-pointers (a multiple of 16, <= %d)", lds_bp_bytes, TTS_EDIT_LDS_BP_BYTES);
  TTS_CHECK_ARG(scratch_bytes >= 0 && (scratch || scratch_bytes == 0), "edit_distance: %lld bytes of scratch without a buffer", scratch_bytes);
  for (int b = 0; b < n; ++b) {
    const TtsPronUtt& q = host[b];
    const long long cap = q.n_frames < E_MAX_HYP ? q.n_frames : E_MAX_HYP;
    if (int rc = check_bp_slot("edit_distance", b, 4 * bp_words(q.n_ref, (int)cap), q.scratch_off, lds_bp_bytes, scratch_bytes)) return rc;
  }
  const int rc = upload_utts("edit_distance", host, dev, n, rows, n_ref_total, TTS_EDIT_MAX_REF, st);
  if (rc != TTS_OK) return rc;
  hipLaunchKernelGGL(edit_distance_kernel, dim3(n), dim3(P_THREADS), (size_t)lds_bp_bytes, st, ref_ids, hyp_id, n_hyp, dev, scratch, counts,
                     ref_to_hyp, hyp_to_ref);
  return launch_status("edit_distance");
}

int phone_posteriors(const float* logits, int rows, int ld, int S, const int* durations, const int* token_ids, int n_tokens_total,
                     const TtsPronUtt* host, TtsPronUtt* dev, int n, float* out, hipStream_t st) {
  TTS_CHECK_ARG(n >= 0 && n_tokens_total >= 0, "phone_posteriors: %d utterances, %d tokens", n, n_tokens_total);
  if (n == 0) return TTS_OK;
  const int rc0 = check_logits("phone_posteriors", logits, rows, ld, S, 0);
  if (rc0 != TTS_OK) return rc0;
  TTS_CHECK_ARG(durations && token_ids && host && dev && out, "phone_posteriors: null pointer");
  const int rc = upload_utts("phone_posteriors", host, dev, n, rows, n_tokens_total, 0x7fffffff, st);
  if (rc != TTS_OK) return rc;
  hipLaunchKernelGGL(phone_posteriors_kernel, dim3(n), dim3(P_THREADS), 0, st, logits, ld, S, durations, token_ids, dev, out);
  return launch_status("phone_posteriors");
}

}  // namespace tts

extern "C" {
int tts_ctc_best_path(const float* logits, int32_t rows, int32_t ld, int32_t n_symbols, int32_t blank, const uint8_t* drop,
                      const TtsPronUtt* utts_host, TtsPronUtt* utts_dev, int32_t n_utts, int32_t* hyp_id, int32_t* hyp_first,
                      int32_t* hyp_last, float* hyp_conf, int32_t* n_hyp, tts_stream_t stream) {
  return tts::ctc_best_path(logits, rows, ld, n_symbols, blank, drop, utts_host, utts_dev, n_utts, hyp_id, hyp_first, hyp_last, hyp_conf, n_hyp,
                            reinterpret_cast<hipStream_t>(stream));
}
int tts_ctc_beam_search(const float* logits, int32_t rows, int32_t ld, int32_t n_symbols, int32_t blank, const uint8_t* drop,
                        const TtsPronUtt* utts_host, TtsPronUtt* utts_dev, int32_t n_utts, int32_t beam, int32_t* scratch,
                        int64_t scratch_words, int32_t* hyp_id, int32_t* n_hyp, double* score, tts_stream_t stream) {
  return tts::ctc_beam_search(logits, rows, ld, n_symbols, blank, drop, utts_host, utts_dev, n_utts, beam, scratch, scratch_words, hyp_id, n_hyp,
                              score, reinterpret_cast<hipStream_t>(stream));
}
int tts_edit_distance(const int32_t* ref_ids, int32_t n_ref_total, const int32_t* hyp_id, int32_t rows, const int32_t* n_hyp,
                      const TtsPronUtt* utts_host, TtsPronUtt* utts_dev, int32_t n_utts, uint8_t* scratch, int64_t scratch_bytes,
                      int32_t lds_bp_bytes, int32_t* counts, int32_t* ref_to_hyp, int32_t* hyp_to_ref, tts_stream_t stream) {
  return tts::edit_distance(ref_ids, n_ref_total, hyp_id, rows, n_hyp, utts_host, utts_dev, n_utts, scratch, scratch_bytes, lds_bp_bytes, counts,
                            ref_to_hyp, hyp_to_ref, reinterpret_cast<hipStream_t>(stream));
}
int tts_phone_posteriors(const float* logits, int32_t rows, int32_t ld, int32_t n_symbols, const int32_t* durations,
                         const int32_t* token_ids, int32_t n_tokens_total, const TtsPronUtt* utts_host, TtsPronUtt* utts_dev,
                         int32_t n_utts, float* out, tts_stream_t stream) {
  return tts::phone_posteriors(logits, rows, ld, n_symbols, durations, token_ids, n_tokens_total, utts_host, utts_dev, n_utts, out,
                               reinterpret_cast<hipStream_t>(stream));
}
}
