// Comparing a synthesised utterance with a recording of the same sentence (DESIGN.md section 16 holds the definition):
//
//   tts_mel_cepstra     per log-mel row: the DCT-II coefficients c1 .. cK in fp64, rounded once to fp32
//   tts_dtw             per pair: dynamic time warping of two cepstral sequences, the path and its cost
//   tts_dtw_path_sums   per pair: the fp64 sums along the path behind MCD, F0 RMSE, log-F0 correlation, GPE, VDE and FFE
//
// Batch independence: every kernel computes a pair (a row) in an order that depends on that pair alone; the reductions are fixed
// trees, there are no atomics and no workgroup waits on another one.
#include "common.h"
#include "pair_sweep.h"
#include "../../include/toucan_compare.h"

namespace tts {

constexpr int C_MELS = TTS_COMPARE_MELS;
constexpr int C_MAX_CEP = TTS_COMPARE_MAX_CEP;
constexpr int C_THREADS = 256;
constexpr int C_ROWS = C_THREADS / C_MAX_CEP;  // 8 log-mel rows per workgroup, one thread per (row, coefficient)

// ---- cepstra -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(C_THREADS) void mel_cepstra_kernel(const float* __restrict__ logmel, int ld, int n_src_rows,
                                                                const int* __restrict__ src_row, int rows, const double* __restrict__ table,
                                                                int K, float* __restrict__ cep) {
  __shared__ double tab[C_MELS * C_MAX_CEP];  // transposed, [m][k]: the threads of a row read neighbouring words
  __shared__ float mel[C_ROWS][C_MELS];
  __shared__ int src[C_ROWS];
  const int tid = threadIdx.x, r = tid / C_MAX_CEP, k = tid % C_MAX_CEP;
  const int row0 = blockIdx.x * C_ROWS;
  for (int e = tid; e < K * C_MELS; e += C_THREADS) {
    const int kk = e / C_MELS, m = e - kk * C_MELS;
    tab[m * K + kk] = table[e];
  }
  if (tid < C_ROWS) {
    const int row = row0 + tid;
    int s = -1;
    if (row < rows) {
      s = src_row ? src_row[row] : row;
      if (s < 0 || s >= n_src_rows) s = -1;
    }
    src[tid] = s;
  }
  __syncthreads();
  for (int e = tid; e < C_ROWS * C_MELS; e += C_THREADS) {
    const int rr = e / C_MELS, m = e - rr * C_MELS;
    mel[rr][m] = src[rr] >= 0 ? logmel[(size_t)src[rr] * ld + m] : 0.0f;
  }
  __syncthreads();
  const int row = row0 + r;
  if (row >= rows || k >= K) return;
  // m in index order, the rounding error of every product (fma) and of every addition (two-sum) carried along in `err`: a flat
  // log-mel (silence) cancels to ~1e-16 of its terms, where a plain fp64 sum would return its own rounding noise
  double acc = 0.0, err = 0.0;
  {
#pragma clang fp contract(off)
    for (int m = 0; m < C_MELS; ++m) {
      const double x = (double)mel[r][m], t = tab[m * K + k];
      const double prod = x * t;
      const double prod_err = __builtin_fma(x, t, -prod);
      const double sum = acc + prod;
      const double part = sum - acc;
      const double sum_err = (acc - (sum - part)) + (prod - part);
      acc = sum;
      err += sum_err + prod_err;
    }
    acc += err;
  }
  cep[(size_t)row * K + k] = src[r] >= 0 ? (float)acc : __builtin_nanf("");
}

int mel_cepstra(const float* logmel, int ld, int n_src_rows, const int* src_row, int rows, const double* table, int K, float* cep,
                hipStream_t st) {
  TTS_CHECK_ARG(logmel && table && cep, "mel_cepstra: null pointer");
  TTS_CHECK_ARG(K >= 1 && K <= C_MAX_CEP, "mel_cepstra: %d coefficients (1 .. %d)", K, C_MAX_CEP);
  TTS_CHECK_ARG(rows >= 0 && n_src_rows >= 0 && ld >= C_MELS, "mel_cepstra: rows %d, source rows %d, row stride %d (>= %d)", rows, n_src_rows,
                ld, C_MELS);
  TTS_CHECK_ARG(src_row || rows <= n_src_rows, "mel_cepstra: %d rows of %d source rows without an index", rows, n_src_rows);
  if (rows == 0) return TTS_OK;
  hipLaunchKernelGGL(mel_cepstra_kernel, dim3((rows + C_ROWS - 1) / C_ROWS), dim3(C_THREADS), 0, st, logmel, ld, n_src_rows, src_row, rows,
                     table, K, cep);
  return launch_status("mel_cepstra");
}

// ---- dynamic time warping, one workgroup per pair ----------------------------------------------------------------------------
// The sweep of pair_sweep.h over fp64 costs: thread t keeps a[i] in registers and b[j] streams (the next row of b is loaded a step
// ahead); a cell adds its distance d to the chosen predecessor, which does not exist outside the matrix (infinite borders; cell
// (0, 0) is d alone).  Thread 0 then walks back from the last cell into row[] (free by then) and the workgroup writes the path
// forwards.
constexpr int D_THREADS = SWEEP_THREADS;
constexpr int D_MAX = TTS_DTW_MAX_FRAMES;
constexpr int D_ROW_BYTES = D_MAX * 8;                 // row[]: fp64 D of a band's last row; then the path, one 32-bit word per point
constexpr int D_DIAG_BYTES = 2 * D_THREADS * 8;
constexpr int D_FIXED_BYTES = D_ROW_BYTES + D_DIAG_BYTES + 16;  // + one slot for the path length; the back-pointers follow
static_assert(2 * D_MAX - 1 <= D_ROW_BYTES / 4, "the path fits where the band row was");
static_assert(D_FIXED_BYTES % 16 == 0 && D_FIXED_BYTES + TTS_DTW_LDS_BP_BYTES <= 160 * 1024, "LDS budget");

template <int KP>
struct DtwCells {
  using value_t = double;
  static constexpr int ORIGIN = 0;
  const float *A, *B;
  int K, Tb;
  double* cost;
  float av[KP], bn[KP], bc[KP];  // a[i]; b of the next step and of this one

  __device__ __forceinline__ void band(int i, bool active) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      av[k] = (active && k < K) ? A[(size_t)i * K + k] : 0.0f;
      bn[k] = (active && threadIdx.x == 0 && k < K) ? B[k] : 0.0f;  // thread 0 starts at step 0 with b[0]
    }
  }
  __device__ __forceinline__ double border(int, int) const { return __builtin_huge_val(); }
  __device__ __forceinline__ void step(int j, bool active) {
#pragma unroll
    for (int k = 0; k < KP; ++k) bc[k] = bn[k];
    const int jn = j + 1;  // the row of b for the next step, loaded now
    if (active && jn >= 0 && jn < Tb) {
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) bn[k] = B[(size_t)jn * K + k];
    }
  }
  __device__ __forceinline__ double via(unsigned int, double pred, int) const { return pred; }
  __device__ __forceinline__ double cell(int i, int j, double best) const {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      if (k < K) {
        const double df = (double)av[k] - (double)bc[k];
        acc += df * df;
      }
    }
    const double d = sqrt(acc);
    return (i == 0 && j == 0) ? d : d + best;
  }
  __device__ __forceinline__ void last(double D) const { *cost = D; }
};

template <int KP>
__global__ __launch_bounds__(D_THREADS) void dtw_kernel(const float* __restrict__ cep_a, const float* __restrict__ cep_b, int K,
                                                        const TtsDtwPair* __restrict__ pairs, unsigned char* __restrict__ scratch,
                                                        int* __restrict__ path, int* __restrict__ path_len, double* __restrict__ cost) {
  extern __shared__ __align__(16) unsigned char lds[];
  double* row = reinterpret_cast<double*>(lds);
  double* diag = reinterpret_cast<double*>(lds + D_ROW_BYTES);
  int* n_points = reinterpret_cast<int*>(lds + D_ROW_BYTES + D_DIAG_BYTES);
  const int p = blockIdx.x, tid = threadIdx.x;
  const TtsDtwPair pr = pairs[p];
  const int Ta = pr.frames_a, Tb = pr.frames_b, W = (Tb + 15) >> 4;
  DtwCells<KP> cells = {cep_a + (size_t)pr.begin_a * K, cep_b + (size_t)pr.begin_b * K, K, Tb, cost + p};
  const unsigned int* bp = pair_sweep(cells, Ta, Tb, row, diag, pr.scratch_off, lds + D_FIXED_BYTES, scratch);
  unsigned int* points = reinterpret_cast<unsigned int*>(lds);  // row[] is free: the path backwards, (i << 16) | j
  if (tid == 0) {
    int i = Ta - 1, j = Tb - 1, n = 0;
    for (;;) {
      points[n++] = ((unsigned int)i << 16) | (unsigned int)j;
      if (i == 0 && j == 0) break;
      unsigned int code = bp_code(bp, W, i, j);
      if (i == 0) code = 2;       // (what the sweep stored there anyway: no other neighbour exists)
      else if (j == 0) code = 1;
      if (code == 0) {
        --i;
        --j;
      } else if (code == 1) {
        --i;
      } else {
        --j;
      }
    }
    *n_points = n;  // every step lowers i + j: n <= Ta + Tb - 1
  }
  __syncthreads();
  const int P = *n_points;
  int* out = path + 2 * (size_t)pr.path_begin;
  for (int q = tid; q < P; q += D_THREADS) {
    const unsigned int e = points[P - 1 - q];
    out[2 * (size_t)q] = (int)(e >> 16);
    out[2 * (size_t)q + 1] = (int)(e & 0xffffu);
  }
  if (tid == 0) path_len[p] = P;
}

// checks the host table, then copies it to the device on the stream
int upload_pairs(const char* what, const TtsDtwPair* host, TtsDtwPair* dev, int n_pairs, int rows_a, int rows_b, long long path_entries,
                 bool with_store, long long scratch_bytes, int lds_bp_bytes, hipStream_t st) {
  for (int p = 0; p < n_pairs; ++p) {
    const TtsDtwPair& q = host[p];
    TTS_CHECK_ARG(q.frames_a >= 1 && q.frames_a <= D_MAX && q.frames_b >= 1 && q.frames_b <= D_MAX,
                  "%s: pair %d has %d x %d frames (1 .. %d per side)", what, p, q.frames_a, q.frames_b, D_MAX);
    TTS_CHECK_ARG(q.begin_a >= 0 && (long long)q.begin_a + q.frames_a <= rows_a && q.begin_b >= 0 && (long long)q.begin_b + q.frames_b <= rows_b,
                  "%s: pair %d lies outside the cepstra (rows %d + %d of %d, %d + %d of %d)", what, p, q.begin_a, q.frames_a, rows_a, q.begin_b,
                  q.frames_b, rows_b);
    TTS_CHECK_ARG(q.path_begin >= 0 && q.path_begin + q.frames_a + q.frames_b - 1 <= path_entries,
                  "%s: pair %d: its path slot (%lld + %d) lies outside the %lld path entries", what, p, (long long)q.path_begin,
                  q.frames_a + q.frames_b - 1, path_entries);
    if (!with_store) continue;
    if (int rc = check_bp_slot(what, p, 4 * bp_words(q.frames_a, q.frames_b), q.scratch_off, lds_bp_bytes, scratch_bytes)) return rc;
  }
  const hipError_t e = hipMemcpyAsync(dev, host, (size_t)n_pairs * sizeof(TtsDtwPair), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) {
    set_error("%s: copying the pair table: %s", what, hipGetErrorString(e));
    return TTS_E_LAUNCH;
  }
  return TTS_OK;
}

template <int KP>
int dtw_launch(const float* cep_a, const float* cep_b, int K, const TtsDtwPair* pairs, int n_pairs, unsigned char* scratch, int lds_bp_bytes,
               int* path, int* path_len, double* cost, hipStream_t st) {
  const size_t lds = (size_t)D_FIXED_BYTES + (size_t)lds_bp_bytes;
  static unsigned long long lds_raised = 0;
  if (lds > 64 * 1024 && raise_lds_limit(reinterpret_cast<const void*>(dtw_kernel<KP>), lds_raised) != hipSuccess) {
    set_error("dtw: raising the dynamic LDS limit failed");
    return TTS_E_LAUNCH;
  }
  hipLaunchKernelGGL(dtw_kernel<KP>, dim3(n_pairs), dim3(D_THREADS), lds, st, cep_a, cep_b, K, pairs, scratch, path, path_len, cost);
  return launch_status("dtw");
}

int dtw(const float* cep_a, int rows_a, const float* cep_b, int rows_b, int K, const TtsDtwPair* pairs_host, TtsDtwPair* pairs_dev, int n_pairs,
        unsigned char* scratch, long long scratch_bytes, int lds_bp_bytes, int* path, long long path_entries, int* path_len, double* cost,
        hipStream_t st) {
  TTS_CHECK_ARG(n_pairs >= 0 && K >= 1 && K <= C_MAX_CEP, "dtw: %d pairs, %d coefficients (1 .. %d)", n_pairs, K, C_MAX_CEP);
  if (n_pairs == 0) return TTS_OK;
  TTS_CHECK_ARG(cep_a && cep_b && pairs_host && pairs_dev && path && path_len && cost, "dtw: null pointer");
  TTS_CHECK_ARG(lds_bp_bytes >= 0 && lds_bp_bytes <= TTS_DTW_LDS_BP_BYTES && lds_bp_bytes % 16 == 0,
                "dtw: %d bytes of LDS for back-pointers (a multiple of 16, <= %d)", lds_bp_bytes, TTS_DTW_LDS_BP_BYTES);
  TTS_CHECK_ARG(scratch_bytes >= 0 && (scratch || scratch_bytes == 0), "dtw: %lld bytes of scratch without a buffer", scratch_bytes);
  const int rc = upload_pairs("dtw", pairs_host, pairs_dev, n_pairs, rows_a, rows_b, path_entries, true, scratch_bytes, lds_bp_bytes, st);
  if (rc != TTS_OK) return rc;
  return K <= 16 ? dtw_launch<16>(cep_a, cep_b, K, pairs_dev, n_pairs, scratch, lds_bp_bytes, path, path_len, cost, st)
                 : dtw_launch<32>(cep_a, cep_b, K, pairs_dev, n_pairs, scratch, lds_bp_bytes, path, path_len, cost, st);
}

// ---- sums along the path, one workgroup per pair -------------------------------------------------------------------------------
constexpr int S_THREADS = 256;
constexpr int S_N = TTS_DTW_N_SUMS;

__global__ __launch_bounds__(S_THREADS) void dtw_path_sums_kernel(const float* __restrict__ cep_a, const float* __restrict__ cep_b, int K,
                                                                  const TtsDtwPair* __restrict__ pairs, const int* __restrict__ path,
                                                                  const int* __restrict__ path_len, const float* __restrict__ f0_a,
                                                                  const float* __restrict__ f0_b, double* __restrict__ sums) {
  __shared__ double red[S_THREADS];
  __shared__ int bad;
  const int p = blockIdx.x, tid = threadIdx.x;
  const TtsDtwPair pr = pairs[p];
  const int Ta = pr.frames_a, Tb = pr.frames_b, P = path_len[p];
  const int* pts = path + 2 * (size_t)pr.path_begin;
  double* out = sums + (size_t)p * S_N;
  if (P < 1 || P > Ta + Tb - 1) {  // (the same decision in every thread)
    if (tid < S_N) out[tid] = __builtin_nan("");
    return;
  }
  if (tid == 0) bad = 0;
  __syncthreads();
  double acc[S_N];
#pragma unroll
  for (int c = 0; c < S_N; ++c) acc[c] = 0.0;
  for (int q = tid; q < P; q += S_THREADS) {
    const int i = pts[2 * (size_t)q], j = pts[2 * (size_t)q + 1];
    if (i < 0 || i >= Ta || j < 0 || j >= Tb) {
      bad = 1;
      continue;
    }
    const float* a = cep_a + ((size_t)pr.begin_a + i) * K;
    const float* b = cep_b + ((size_t)pr.begin_b + j) * K;
    double d2 = 0.0;
    for (int k = 0; k < K; ++k) {
      const double df = (double)a[k] - (double)b[k];
      d2 += df * df;
    }
    acc[TTS_DTW_SUM_MCD] += sqrt(2.0 * d2);
    if (q > 0 && i - pts[2 * (size_t)q - 2] == 1 && j - pts[2 * (size_t)q - 1] == 1) acc[TTS_DTW_SUM_DIAG] += 1.0;
    if (f0_a && f0_b) {
      const double fa = (double)f0_a[(size_t)pr.begin_a + i], fb = (double)f0_b[(size_t)pr.begin_b + j];
      const bool va = fa > 0.0, vb = fb > 0.0;
      if (va && vb) {
        const double dh = fa - fb, cents = 1200.0 * log2(fa / fb), x = log(fa), y = log(fb);
        acc[TTS_DTW_SUM_VV] += 1.0;
        acc[TTS_DTW_SUM_SQ_HZ] += dh * dh;
        acc[TTS_DTW_SUM_SQ_CENTS] += cents * cents;
        acc[TTS_DTW_SUM_X] += x;
        acc[TTS_DTW_SUM_Y] += y;
        acc[TTS_DTW_SUM_XX] += x * x;
        acc[TTS_DTW_SUM_YY] += y * y;
        acc[TTS_DTW_SUM_XY] += x * y;
        if (fabs(dh) > 0.2 * fb) acc[TTS_DTW_SUM_GROSS] += 1.0;
      } else if (va != vb) {
        acc[TTS_DTW_SUM_VUV] += 1.0;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < S_N; ++c) {  // a fixed tree over the 256 partial sums
    red[tid] = acc[c];
    __syncthreads();
    for (int o = S_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) acc[c] = red[0];
    __syncthreads();
  }
  if (tid == 0) {
    const bool nan_row = bad != 0;  // (the barriers of the tree have published every thread's flag)
    for (int c = 0; c < S_N; ++c) out[c] = nan_row ? __builtin_nan("") : acc[c];
  }
}

int dtw_path_sums(const float* cep_a, int rows_a, const float* cep_b, int rows_b, int K, const TtsDtwPair* pairs_host, TtsDtwPair* pairs_dev,
                  int n_pairs, const int* path, long long path_entries, const int* path_len, const float* f0_a, const float* f0_b, double* sums,
                  hipStream_t st) {
  TTS_CHECK_ARG(n_pairs >= 0 && K >= 1 && K <= C_MAX_CEP, "dtw_path_sums: %d pairs, %d coefficients (1 .. %d)", n_pairs, K, C_MAX_CEP);
  if (n_pairs == 0) return TTS_OK;
  TTS_CHECK_ARG(cep_a && cep_b && pairs_host && pairs_dev && path && path_len && sums, "dtw_path_sums: null pointer");
  TTS_CHECK_ARG((f0_a == nullptr) == (f0_b == nullptr), "dtw_path_sums: f0 of one side only");
  const int rc = upload_pairs("dtw_path_sums", pairs_host, pairs_dev, n_pairs, rows_a, rows_b, path_entries, false, 0, 0, st);
  if (rc != TTS_OK) return rc;
  hipLaunchKernelGGL(dtw_path_sums_kernel, dim3(n_pairs), dim3(S_THREADS), 0, st, cep_a, cep_b, K, pairs_dev, path, path_len, f0_a, f0_b, sums);
  return launch_status("dtw_path_sums");
}

}  // namespace tts

extern "C" {
int tts_dtw_max_frames(void) { return TTS_DTW_MAX_FRAMES; }
int tts_mel_cepstra(const float* logmel, int32_t ld, int32_t n_src_rows, const int32_t* src_row, int32_t rows, const double* table,
                    int32_t n_cep, float* cep, tts_stream_t stream) {
  return tts::mel_cepstra(logmel, ld, n_src_rows, src_row, rows, table, n_cep, cep, reinterpret_cast<hipStream_t>(stream));
}
int tts_dtw(const float* cep_a, int32_t rows_a, const float* cep_b, int32_t rows_b, int32_t n_cep, const TtsDtwPair* pairs_host,
            TtsDtwPair* pairs_dev, int32_t n_pairs, uint8_t* scratch, int64_t scratch_bytes, int32_t lds_bp_bytes, int32_t* path,
            int64_t path_entries, int32_t* path_len, double* cost, tts_stream_t stream) {
  return tts::dtw(cep_a, rows_a, cep_b, rows_b, n_cep, pairs_host, pairs_dev, n_pairs, scratch, scratch_bytes, lds_bp_bytes, path, path_entries,
                  path_len, cost, reinterpret_cast<hipStream_t>(stream));
}
int tts_dtw_path_sums(const float* cep_a, int32_t rows_a, const float* cep_b, int32_t rows_b, int32_t n_cep, const TtsDtwPair* pairs_host,
                      TtsDtwPair* pairs_dev, int32_t n_pairs, const int32_t* path, int64_t path_entries, const int32_t* path_len,
                      const float* f0_a, const float* f0_b, double* sums, tts_stream_t stream) {
  return tts::dtw_path_sums(cep_a, rows_a, cep_b, rows_b, n_cep, pairs_host, pairs_dev, n_pairs, path, path_entries, path_len, f0_a, f0_b, sums,
                            reinterpret_cast<hipStream_t>(stream));
}
}
