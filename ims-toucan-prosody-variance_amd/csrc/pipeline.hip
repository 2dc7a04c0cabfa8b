// Stage-level entry points of libtoucan_hip.so: a handle that owns the packed weights and the workspace, and C++ functions that
// sequence the kernels of one stage of the reference's forward pass (declared in include/toucan_tts.h, "stage API").
//
// This is the native counterpart of the launch sequencing in engine.py: same kernels, same order, same buffers' roles - a pass
// is a handful of calls through the C ABI instead of ~500.  Mirrors, stage by stage:
//   tts_encoder               Conformer.forward (Layers/Conformer.py:92-134) on the phoneme features
//   tts_variance_predictors   VariancePredictor.forward / DurationPredictor.inference (VariancePredictor.py:65-80, DurationPredictor.py:63-83)
//   tts_control_and_regulate  InferenceToucanTTS.py:214-235 (+ _scale_variance :333-343, LengthRegulator.py:37-61)
//   tts_control_and_regulate_v  the same with per-utterance scales and the statistics around them (include/toucan_prosody.h)
//   tts_control_and_regulate_c  the same with a per-phoneme curve table and span statistics (include/toucan_prosody_curves.h)
//   tts_control_and_regulate_t  the same with utterances, pauses or spans fitted to a number of frames (include/toucan_prosody_fit.h)
//   tts_teacher_forced        the scorer's replacement of the two above: ToucanTTS.py:321-330 (include/toucan_score.h)
//   tts_decoder               decoder Conformer + feat_out (InferenceToucanTTS.py:238-239)
//   tts_postnet               PostNet.forward + residual (PostNet.py:62-74, InferenceToucanTTS.py:241)
//   tts_postflow              Glow.forward(infer=True) (Glow.py:342-391)
//   tts_postflow_nll          Glow.forward(infer=False): the scorer's glow loss (include/toucan_score.h)
//   tts_vocoder_bigvgan/_hifigan  InferenceBigVGAN.py:72-95 / InferenceAvocodo.py:69-80
//   tts_synthesize_batch      all of the above for one ragged batch
// Host work here is layout arithmetic (tile tables, offsets) and launch ordering; every FLOP is in the kernels.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "common.h"
#include "../../include/toucan_prosody.h"
#include "../../include/toucan_prosody_curves.h"
#include "../../include/toucan_prosody_fit.h"
#include "../../include/toucan_score.h"

namespace tts {

const char* conv1d_wide_reject(const TtsConvDesc& d);  // conv1d_wide.hip: nullptr when the call may take the wide form

namespace {

constexpr int ATT = 192, HEADS = 4, DK = 48;

struct Dev {
  void* p = nullptr;
  int64_t shape[4] = {0, 0, 0, 0};
  int ndim = 0, dtype = 0;
  size_t bytes = 0;
};

struct ConvW {
  const float* w = nullptr;
  const void* w16 = nullptr;
  const float* bias = nullptr;
  int mode = 0, taps = 1, dil = 1, pad_left = 0, cin = 0, cin_pad = 0, cout = 0, wn = 0, half_pad = 0, tile_rows = 0, small_tile_rows = 0,
      small_only = 0, n_tile = 0, compute16 = 0, algo_taps = 1;
};

// ---- the model: one field per tensor the stages use, resolved from the weight table once (resolve_acoustic / resolve_vocoder) ----
struct Block {  // one Conformer block
  const float *ln_g[5], *ln_b[5];  // norm_ff_macaron, norm_mha, norm_conv, norm_ff, norm_final
  ConvW ffm1, ffm2, qkv, out, pos, pw1, pw2, ff1, ff2;
  const float *u, *v, *dw_w, *dw_b;
  const Dev *ffm_fused = nullptr, *ff_fused = nullptr;  // packing.pack_ffn (16-bit configurations, kernel size 1), or null
};

struct Predictor {
  int layers = 0, first_cln = 0;  // conditional layer norms are numbered pitch 0..6, energy 7..8, duration 9..11 (engine.py packs them so)
  ConvW conv[7], lin;
  const float *g[7], *b[7];  // plain LayerNorms of the single-speaker checkpoint
};

struct Acoustic {
  bool resolved = false;
  ConvW embed0, embed2;
  const float* lang_table = nullptr;  // null when absent: an error only where language ids are passed
  Block enc[6], dec[6];
  const float *out_norm_g, *out_norm_b;
  ConvW hs_h, hs_e;  // multi-speaker checkpoints only, like cln_weights
  const float* cln_weights = nullptr;
  int n_mlp = 0;
  Predictor pitch, energy, duration;
  const float *pitch_w, *pitch_b, *energy_w, *energy_b;
  ConvW feat_out, g_proj;
  struct { ConvW conv; const float *g, *b; } postnet[5];
  struct { ConvW start, end, cond; const float *winv, *an_bias, *an_logs; } flow[18];
  // the forward direction (tts_postflow_nll), present in a scoring pipeline only: the InvConvNear weight itself, the `end` conv packed
  // as a plain conv that writes [m | logs], and the constant part of a row's log-determinant
  bool scoring = false;
  struct { const float* wfwd; ConvW end_ml; } flow_fwd[18];
  double flow_logdet = 0.0;
  struct { ConvW inl[4], res_skip[4]; } flowgrp[5];  // in / res-skip layers are shared inside groups of 4 blocks (Glow.py:325-327)
};

struct Vocoder {
  bool resolved = false;
  ConvW pre, ups[4];
  struct { ConvW c1, c2; const float *a1 = nullptr, *b1 = nullptr, *a2 = nullptr, *b2 = nullptr; } blk[4][3][3];  // snake parameters: BigVGAN only
  const float *post_w, *post_a = nullptr, *post_b = nullptr, *filt = nullptr;
  const void* fir_tab = nullptr;
};

// packed ragged layout: utterance u occupies rows [begins[u], begins[u] + lengths[u])
struct Layout {
  std::vector<int> begins, lengths;
  int total = 0, max_len = 0;
  static Layout make(const int* len, int n, int align) {
    Layout l;
    int off = 0;
    for (int i = 0; i < n; ++i) {
      l.begins.push_back(off);
      l.lengths.push_back(len[i]);
      off += (len[i] + align - 1) / align * align;
      l.max_len = std::max(l.max_len, len[i]);
    }
    l.total = off;
    return l;
  }
  Layout scaled(int f) const {
    Layout l;
    for (size_t i = 0; i < begins.size(); ++i) {
      l.begins.push_back(begins[i] * f);
      l.lengths.push_back(lengths[i] * f);
    }
    l.total = total * f;
    l.max_len = max_len * f;
    return l;
  }
  Layout halved() const {  // Glow squeeze: an odd last frame is dropped (glow_utils.py:31-32); begins are even by construction
    Layout l;
    for (size_t i = 0; i < begins.size(); ++i) {
      l.begins.push_back(begins[i] / 2);
      l.lengths.push_back(lengths[i] / 2);
      l.max_len = std::max(l.max_len, lengths[i] / 2);
    }
    l.total = total / 2;
    return l;
  }
  int n() const { return (int)lengths.size(); }
};

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0;
  void reset() { off = 0; }
};

struct TileTab {
  TtsTile* dev = nullptr;
  int n = 0;
};

// Tile tables / utterance bounds of a group of stages (acoustic stages, or the vocoder) in one of its two generations, which
// alternate from batch to batch.  Append-only: a table is copied into pinned staging and uploaded with one asynchronous copy on the
// stage's stream, into a chunk that is never moved or freed before tts_destroy - an address handed out stays valid.  A generation
// keeps its tables from batch to batch (a repeating layout is found, not uploaded again) until it holds more than TABLE_BUDGET bytes:
// then the next batch that takes it rewinds it, once its last use has completed.
constexpr size_t TABLE_FIRST_CHUNK = 64 << 10;
constexpr size_t TABLE_BUDGET = 16 << 20;

struct TableChunk {
  char* dev = nullptr;
  char* host = nullptr;  // staging, same size
  size_t cap = 0, off = 0;
};

struct TableStore {
  std::vector<TableChunk> chunks;
  std::unordered_map<std::string, std::pair<void*, int>> index;  // layout key -> device address, element count
  hipEvent_t last_use = nullptr;  // recorded on its stream at the end of every stage entry of the group (the extern "C" wrappers)
};

// one timed launch of the roofline leg (tts_profile): HIP events on the launch stream around a matrix-core kernel
struct ProfRec {
  std::string name;
  double flops = 0, bytes = 0, elems = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

}  // namespace

struct Handle {
  TtsConfig cfg;
  std::unordered_map<std::string, Dev> weights;
  Acoustic acoustic;  // resolved at the top of tts_encoder, vocoder at the top of tts_vocoder_*; tts_load_weights unresolves both
  Vocoder vocoder;
  Arena phone, frame, voc[2];
  Arena nll;                      // tts_postflow_nll's own scratch (outside tts_workspace_bytes: synthesis handles never claim it)
  TableStore tabs[2][2];          // [0: acoustic stages, 1: vocoder][generation]
  int tab_gen[2] = {0, 0};
  int tab_which = 0;              // group of the stage entry that runs (set with split_mode)
  long long n_tables_built = 0;   // (tts_table_stats)
  int small_tile_blocks = 1536;
  int split_mode = 0;             // set by the stage entries; the fp32 configuration only.  2 (phoneme stages: encoder, predictors): split-K convs
                                  // and key-split attention at EVERY grid size - durations are a rounding of exp(log d), so everything upstream
                                  // of them keeps one arithmetic whatever the batch (an utterance's frame count cannot depend on the batch or
                                  // shard it is in); 1 (frame stages): the split forms on small grids only (TTS_IO_SPLIT_K / TTS_ATT_KEY_SPLIT:
                                  // the mel agrees to rounding order across batch sizes); 0 (vocoder: chunked == whole, bit for bit)
  // relative position tables [block][2 pmax - 1][192] of the two Conformer stacks, built from the uploaded sinusoid table
  float* ptab[2] = {nullptr, nullptr};
  int pmax = 0;
  // state of the batch in flight
  Layout lp, lf;          // phoneme and frame layouts
  int B = 0;
  const float* text = nullptr;
  float *e_norm = nullptr, *enc = nullptr, *pitch = nullptr, *energy = nullptr, *cln = nullptr;
  int* dur = nullptr;
  float *cat = nullptr, *dec = nullptr, *mel0 = nullptr, *mel = nullptr;
  std::vector<int> frames;  // per utterance, after the control step
  float* pstats = nullptr;           // in the phoneme arena, room for B + R rows twice: [before | after][B][TTS_PROSODY_STATS], then
                                     // [before | after][n_spans][TTS_PROSODY_STATS] (tts_control_and_regulate_v and _c)
  std::vector<float> pstats_host;    // the utterance blocks, read back with the durations; empty if the batch went through the scalar entry
  int n_spans = -1;                  // spans of the last tts_control_and_regulate_c of the batch in flight; -1: it did not run
  std::vector<float> sstats_host;    // [2][n_spans][TTS_PROSODY_STATS], read back with the durations
  float* fit_ws = nullptr;           // in the phoneme arena: scales_out [B][4] | curves_out [R][5] | report [R][8] | extra [R] (tts_control_and_regulate_t)
  int n_fit = -1;                    // segments of the last tts_control_and_regulate_t of the batch in flight; -1: it did not run
  std::vector<float> fit_host;       // its report [n_fit][TTS_FIT_COLUMNS], then the solved scales [B][TTS_PROSODY_SCALES]: read back likewise
  std::vector<int> fit_extra_host;   // and its extra frames [R]
  bool have_flow = false;
  // profiling (bench.py's roofline leg): event pairs around the launches of the selected kernel class ("" = every class)
  bool prof_on = false, prof_detail = false;
  std::string prof_select;
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> event_pool;
};

namespace {

#define TTS_TRY(expr)            \
  do {                           \
    const int rc_ = (expr);      \
    if (rc_ != TTS_OK) return rc_; \
  } while (0)

bool is16(const Handle* h);

// the stages after tts_encoder read the model it resolved: a tts_load_weights call since then (it may have freed a tensor) ends the pass
#define TTS_CHECK_RESOLVED(h, entry) TTS_CHECK_ARG((h)->acoustic.resolved, "%s: weights were loaded since tts_encoder: run it again", entry)

int hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return TTS_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return TTS_E_LAUNCH;
}

// ---- arenas ---------------------------------------------------------------------------------------------------------
int arena_reserve(Arena& a, size_t bytes, hipStream_t st) {
  a.reset();
  if (a.cap >= bytes) return TTS_OK;
  if (a.base) {
    TTS_TRY(hip_ok(hipStreamSynchronize(st), "workspace: stream sync before regrowth"));
    (void)hipFree(a.base);
    a.base = nullptr;
    a.cap = 0;
  }
  const size_t want = bytes + bytes / 8 + (1 << 20);  // (= with_growth_slack(bytes): tts_workspace_bytes counts it)
  TTS_TRY(hip_ok(hipMalloc(reinterpret_cast<void**>(&a.base), want), "workspace: hipMalloc"));
  a.cap = want;
  return TTS_OK;
}

template <class T>
T* arena_alloc(Arena& a, size_t count) {
  const size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
  if (a.off + bytes > a.cap) return nullptr;
  T* p = reinterpret_cast<T*>(a.base + a.off);
  a.off += bytes;
  return p;
}

#define TTS_ALLOC(var, arena, T, count)                                                        \
  T* var = arena_alloc<T>(arena, (size_t)(count));                                             \
  if (!var) {                                                                                  \
    set_error("%s: workspace exhausted (%zu of %zu bytes used)", __func__, (arena).off, (arena).cap); \
    return TTS_E_ARG;                                                                          \
  }

// ---- tile tables and utterance bounds (kept per layout signature) -----------------------------------------------------
std::string layout_key(const Layout& l, int tile_rows) {
  std::string k(reinterpret_cast<const char*>(l.begins.data()), l.begins.size() * sizeof(int));
  k.append(reinterpret_cast<const char*>(l.lengths.data()), l.lengths.size() * sizeof(int));
  k.append(reinterpret_cast<const char*>(&tile_rows), sizeof(int));
  return k;
}

// a stage group starts a batch: take the group's other table generation
int tables_begin(Handle* h, int which, hipStream_t st) {
  h->tab_which = which;
  h->tab_gen[which] ^= 1;
  TableStore& s = h->tabs[which][h->tab_gen[which]];
  if (!s.last_use) return TTS_OK;  // (never used)
  size_t held = 0;
  for (const TableChunk& c : s.chunks) held += c.off;
  if (held > TABLE_BUDGET) {  // rewind: its staging and device bytes are overwritten from here on
    TTS_TRY(hip_ok(hipEventSynchronize(s.last_use), "tile tables: last use before rewinding"));
    s.index.clear();
    for (TableChunk& c : s.chunks) c.off = 0;
    return TTS_OK;
  }
  const hipError_t q = hipEventQuery(s.last_use);
  if (q == hipSuccess) return TTS_OK;
  if (q != hipErrorNotReady) return hip_ok(q, "tile tables: last use");
  (void)hipGetLastError();  // (not-ready is no error: clear it for the launch checks that follow)
  // the tables kept in this generation may have been uploaded on another stream: order this batch behind their last use
  return hip_ok(hipStreamWaitEvent(st, s.last_use, 0), "tile tables: wait for last use");
}

// the table `key` of the running group's current generation.  On a miss build() makes its host elements, which are appended:
// into the first chunk with room, else into a new one twice the size of the last (one staging copy + one upload on st)
template <class Build>
int table_of(Handle* h, const std::string& key, hipStream_t st, Build build, void** dev, int* n) {
  TableStore& s = h->tabs[h->tab_which][h->tab_gen[h->tab_which]];
  auto it = s.index.find(key);
  if (it == s.index.end()) {
    auto host = build();
    const int count = (int)host.size();
    if (host.empty()) host.resize(1);  // (an empty layout still gets a valid address)
    const size_t bytes = host.size() * sizeof(host[0]), need = (bytes + 255) & ~(size_t)255;
    TableChunk* c = nullptr;
    for (TableChunk& k : s.chunks)
      if (k.off + need <= k.cap) {
        c = &k;
        break;
      }
    if (!c) {
      TableChunk k;
      k.cap = std::max(s.chunks.empty() ? TABLE_FIRST_CHUNK : 2 * s.chunks.back().cap, need);
      TTS_TRY(hip_ok(hipMalloc(reinterpret_cast<void**>(&k.dev), k.cap), "tile tables: hipMalloc"));
      const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&k.host), k.cap, hipHostMallocDefault);
      if (e != hipSuccess) (void)hipFree(k.dev);
      TTS_TRY(hip_ok(e, "tile tables: hipHostMalloc"));
      s.chunks.push_back(k);
      c = &s.chunks.back();
    }
    memcpy(c->host + c->off, host.data(), bytes);
    TTS_TRY(hip_ok(hipMemcpyAsync(c->dev + c->off, c->host + c->off, bytes, hipMemcpyHostToDevice, st), "tile tables: upload"));
    it = s.index.emplace(key, std::make_pair(static_cast<void*>(c->dev + c->off), count)).first;
    c->off += need;
    ++h->n_tables_built;
  }
  *dev = it->second.first;
  if (n) *n = it->second.second;
  return TTS_OK;
}

int tiles_of(Handle* h, const Layout& l, int tile_rows, hipStream_t st, TileTab* out) {
  void* dev;
  TTS_TRY(table_of(h, layout_key(l, tile_rows), st, [&] {
    std::vector<TtsTile> host;
    for (int u = 0; u < l.n(); ++u)
      for (int r = 0; r < l.lengths[u]; r += tile_rows) host.push_back(TtsTile{l.begins[u] + r, l.begins[u], l.begins[u] + l.lengths[u], u});
    return host;
  }, &dev, &out->n));
  out->dev = static_cast<TtsTile*>(dev);
  return TTS_OK;
}

// (seq_begin[n] | seq_end[n]) device array
int bounds_of(Handle* h, const Layout& l, hipStream_t st, const int** sb, const int** se) {
  void* dev;
  TTS_TRY(table_of(h, layout_key(l, -1), st, [&] {
    std::vector<int> host(2 * std::max(1, l.n()));
    for (int u = 0; u < l.n(); ++u) {
      host[u] = l.begins[u];
      host[l.n() + u] = l.begins[u] + l.lengths[u];
    }
    return host;
  }, &dev, nullptr));
  *sb = static_cast<const int*>(dev);
  *se = *sb + l.n();
  return TTS_OK;
}

// ---- weights ------------------------------------------------------------------------------------------------------------
const Dev* find(const Handle* h, const std::string& name) {
  auto it = h->weights.find(name);
  return it == h->weights.end() ? nullptr : &it->second;
}

int need(const Handle* h, const std::string& name, const Dev** out) {
  *out = find(h, name);
  if (!*out) {
    set_error("weight '%s' was not loaded (tts_load_weights)", name.c_str());
    return TTS_E_ARG;
  }
  return TTS_OK;
}

int fvec(const Handle* h, const std::string& name, const float** out) {
  const Dev* d;
  TTS_TRY(need(h, name, &d));
  *out = static_cast<const float*>(d->p);
  return TTS_OK;
}

// a packed conv: "<name>.w" (+ ".w16", ".bias") and the host-side descriptor fields in "<name>.meta" (int32[16], kept on the host)
int conv_of(const Handle* h, const std::string& name, ConvW* c) {
  const Dev *w, *m;
  TTS_TRY(need(h, name + ".w", &w));
  TTS_TRY(need(h, name + ".meta", &m));
  const int* mm = static_cast<const int*>(m->p);  // meta tensors live in host memory (dtype 3 is never uploaded)
  c->w = static_cast<const float*>(w->p);
  const Dev* w16 = find(h, name + ".w16");
  c->w16 = w16 ? w16->p : nullptr;
  const Dev* b = find(h, name + ".bias");
  c->bias = b ? static_cast<const float*>(b->p) : nullptr;
  c->mode = mm[0]; c->taps = mm[1]; c->dil = mm[2]; c->pad_left = mm[3]; c->cin = mm[4]; c->cin_pad = mm[5]; c->cout = mm[6];
  c->wn = mm[7]; c->half_pad = mm[8]; c->tile_rows = mm[9]; c->small_tile_rows = mm[10]; c->small_only = mm[11]; c->n_tile = mm[12];
  c->compute16 = mm[13];
  c->algo_taps = mm[14] > 0 ? mm[14] : c->taps;
  return TTS_OK;
}

// ---- profiling hook ---------------------------------------------------------------------------------------------------------
hipEvent_t prof_event(Handle* h) {
  if (!h->event_pool.empty()) {
    hipEvent_t e = h->event_pool.back();
    h->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

// launch() between an event pair on st if the class `name` is being profiled, plainly otherwise; returns launch()'s status
template <class Launch>
int prof_launch(Handle* h, const char* name, double flops, double bytes, double elems, hipStream_t st, Launch launch) {
  if (!h->prof_on || !(h->prof_select.empty() || h->prof_select == name)) return launch();
  h->prof.emplace_back();
  ProfRec* r = &h->prof.back();
  r->name = name; r->flops = flops; r->bytes = bytes; r->elems = elems;
  r->e0 = prof_event(h);
  r->e1 = prof_event(h);
  (void)hipEventRecord(r->e0, st);
  const int rc = launch();
  (void)hipEventRecord(r->e1, st);
  return rc;
}

// ---- one conv launch (engine.Ops.conv) ----------------------------------------------------------------------------------
struct T2 {  // a [rows, cols] view
  void* p;
  int ld;
  int bits;  // 32, or 16 (format = the handle's precision)
  T2() : p(nullptr), ld(0), bits(32) {}
  T2(void* p_, int ld_, int bits_ = 32) : p(p_), ld(ld_), bits(bits_) {}
};

struct ConvOpt {
  int pre = TTS_PRE_NONE;
  float pre_slope = 0.f;
  int act = TTS_ACT_NONE;
  float alpha = 1.f;
  const float* seqvec = nullptr; int ld_seqvec = 0;
  const float* preadd = nullptr; int ld_preadd = 0;
  T2 res; float res_scale = 1.f;
  const float* aux = nullptr; int ld_aux = 0;
  bool accumulate = false;
  bool fp32_only = false;  // run on the fp32 MFMA path even if a 16-bit copy exists
  bool no_split_k = false; // never the split-K form (the position tables: their rows must not depend on the table's size)
  const float *snake_alpha = nullptr, *snake_beta = nullptr, *snake_filt = nullptr;
};

// CUs of the current device (asked once per device)
int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  int& c = cus[dev & 63];
  if (c == 0 && (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 1)) {
    (void)hipGetLastError();
    c = 256;
  }
  return c;
}

int conv(Handle* h, const ConvW& cw, T2 x, T2 y, const Layout& l, hipStream_t st, const ConvOpt& o = ConvOpt()) {
  int tile_rows = cw.tile_rows;
  if (h->small_tile_blocks && cw.small_tile_rows && !cw.small_only) {
    const int cols = cw.mode == TTS_MODE_LINEAR ? cw.wn : cw.half_pad;
    const long long grid = (long long)((l.total + cw.tile_rows - 1) / cw.tile_rows) * (cols / cw.n_tile);
    if (grid < h->small_tile_blocks) tile_rows = cw.small_tile_rows;
  }
  TileTab tt;
  TTS_TRY(tiles_of(h, l, tile_rows, st, &tt));
  TtsConvDesc d;
  memset(&d, 0, sizeof(d));
  bool use16 = !o.fp32_only && h->cfg.precision != TTS_COMPUTE_F32 && cw.w16 != nullptr;
  if (use16 && cw.compute16 == TTS_COMPUTE_F32X3) {
    // the split fp32 product (same rule as engine.Ops.conv): not in the phoneme stages (exact fp32 upstream of the rounded
    // durations), and not where the exact fp32 split-K form is the fast one (frame stages on grids of a few workgroups)
    const int cols = cw.mode == TTS_MODE_LINEAR ? cw.wn : cw.half_pad;
    const bool small = (long long)tt.n * (tile_rows / 64) * ((cols + 63) / 64) <= 128;
    if (h->split_mode == 2 || (h->split_mode == 1 && small)) use16 = false;
  }
  d.x = static_cast<const float*>(x.p); d.ldx = x.ld; d.cin = cw.cin;
  d.w = use16 ? cw.w16 : cw.w; d.cin_pad = cw.cin_pad; d.wn = cw.wn; d.half_pad = cw.half_pad;
  d.bias = cw.bias;
  d.y = static_cast<float*>(y.p); d.ldy = y.ld; d.cout = cw.cout;
  d.taps = cw.taps; d.dil = cw.dil; d.pad_left = cw.pad_left;
  d.pre_act = o.pre; d.pre_slope = o.pre_slope;
  d.snake_alpha = o.snake_alpha; d.snake_beta = o.snake_beta; d.snake_filt = o.snake_filt;
  d.mode = cw.mode; d.act = o.act; d.alpha = o.alpha;
  d.seqvec = o.seqvec; d.ld_seqvec = o.ld_seqvec;
  d.preadd = o.preadd; d.ld_preadd = o.ld_preadd;
  d.res = static_cast<const float*>(o.res.p); d.ld_res = o.res.ld; d.res_scale = o.res_scale;
  d.aux = o.aux; d.ld_aux = o.ld_aux;
  d.accumulate = o.accumulate ? 1 : 0;
  d.compute = use16 ? cw.compute16 : TTS_COMPUTE_F32;
  const bool any16 = x.bits == 16 || y.bits == 16 || (o.res.p && o.res.bits == 16);
  d.io_flags = (x.bits == 16 ? TTS_IO_X_BF16 : 0) | (y.bits == 16 ? TTS_IO_Y_BF16 : 0) | ((o.res.p && o.res.bits == 16) ? TTS_IO_RES_BF16 : 0) |
               ((any16 && h->cfg.precision == TTS_COMPUTE_F16) ? TTS_IO_F16 : 0);
  // the fp32 configuration only: the fp32 layers of a 16-bit configuration keep one accumulation order at every batch size (an
  // utterance's result there does not depend on the batch it is in, bit for bit - tests/test_gpu_e2e.py asserts it)
  if (h->split_mode && !o.no_split_k && !is16(h) && d.compute == TTS_COMPUTE_F32)
    d.io_flags |= h->split_mode == 2 ? TTS_IO_SPLIT_K_ALWAYS : TTS_IO_SPLIT_K;
  if (cw.algo_taps == 2 && cw.taps == 3) d.io_flags |= TTS_IO_POLYPHASE;  // a transposed conv packed as a polyphase conv (packing.pack_conv_transpose)
  // The wide form (256 x 256 tiles, conv1d_wide.hip) where the call is eligible, its grid gives every CU a workgroup and the shape
  // measured faster on it (one workgroup per CU exposes the epilogue, so the contraction has to be long - at
  // least 28 (slab, tap) steps - or the polyphase skip has to drop whole steps, which takes two or more column tiles); the results
  // are bit-identical to the other forms, so this is a speed choice only (same rule as engine.Ops.conv).
  const bool wide_pays = (cw.cin / 64) * cw.taps >= 28 || ((d.io_flags & TTS_IO_POLYPHASE) && cw.wn >= 512);
  if (cw.tile_rows != 256 && wide_pays && conv1d_wide_reject(d) == nullptr) {
    long long t256 = 0;
    for (int n : l.lengths) t256 += (n + 255) / 256;
    if (t256 * (cw.wn / 256) >= device_cus()) {
      tile_rows = 256;
      TTS_TRY(tiles_of(h, l, tile_rows, st, &tt));
    }
  }
  d.tiles = tt.dev; d.n_tiles = tt.n; d.tile_rows = tile_rows;
  if (h->prof_on) {  // same class names and algorithmic work as profiling.py (kernel_class / ConvTimer.add)
    const bool dual = cw.mode != TTS_MODE_LINEAR;
    const bool wide = tile_rows == 256 && cw.tile_rows != 256;
    const int bm = tile_rows != cw.tile_rows ? tile_rows : cw.tile_rows, bn = wide ? 256 : (tile_rows != cw.tile_rows ? 64 : cw.n_tile);
    char name[96];
    int nlen = snprintf(name, sizeof(name), "conv1d_%s<%dx%d%s>", d.compute == TTS_COMPUTE_F32 ? "f32" : (d.compute == TTS_COMPUTE_BF16 ? "bf16" : (d.compute == TTS_COMPUTE_F16 ? "f16" : "f32x3")),
                        bm, bn, dual ? ",dual" : "");
    if (h->prof_detail)  // per-shape classes (tools/conv_shapes.py): where the small-GEMM time goes
      snprintf(name + nlen, sizeof(name) - nlen, "[%dx%d k%d r%d]", cw.cin, cw.cout * (dual ? 2 : 1), cw.taps, l.total);
    double rows = 0;
    for (int n : l.lengths) rows += n;
    const double ctot = (double)cw.cout * (dual ? 2 : 1);
    return prof_launch(h, name, 2.0 * rows * cw.cin * ctot * cw.algo_taps,
                       rows * (cw.cin * (x.bits / 8.0) + cw.cout * (y.bits / 8.0)) + cw.taps * cw.cin * ctot * (d.compute == TTS_COMPUTE_F32 ? 4 : 2),
                       rows * cw.cout, st, [&] { return tts_conv1d(&d, st); });
  }
  return tts_conv1d(&d, st);
}

// ---- the model resolved from the weight table: the only place where tensor names appear ---------------------------------------
// (the counterpart of native.py's _upload_acoustic / _upload_vocoder; a missing tensor is reported here, before a pass enqueues anything)
int block_of(const Handle* h, const std::string& p, Block* b) {
  static const char* ln[5] = {"norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final"};
  for (int i = 0; i < 5; ++i) {
    TTS_TRY(fvec(h, p + ln[i] + ".g", &b->ln_g[i]));
    TTS_TRY(fvec(h, p + ln[i] + ".b", &b->ln_b[i]));
  }
  TTS_TRY(conv_of(h, p + "ffm.w1", &b->ffm1));
  TTS_TRY(conv_of(h, p + "ffm.w2", &b->ffm2));
  TTS_TRY(conv_of(h, p + "ff.w1", &b->ff1));
  TTS_TRY(conv_of(h, p + "ff.w2", &b->ff2));
  b->ffm_fused = find(h, p + "ffm.fused");
  b->ff_fused = find(h, p + "ff.fused");
  TTS_TRY(conv_of(h, p + "qkv", &b->qkv));
  TTS_TRY(conv_of(h, p + "out", &b->out));
  TTS_TRY(conv_of(h, p + "pos", &b->pos));
  TTS_TRY(conv_of(h, p + "pw1", &b->pw1));
  TTS_TRY(conv_of(h, p + "pw2", &b->pw2));
  TTS_TRY(fvec(h, p + "u", &b->u));
  TTS_TRY(fvec(h, p + "v", &b->v));
  TTS_TRY(fvec(h, p + "dw_w", &b->dw_w));
  TTS_TRY(fvec(h, p + "dw_b", &b->dw_b));
  return TTS_OK;
}

int predictor_of(const Handle* h, const std::string& p, int layers, int first_cln, Predictor* out) {
  out->layers = layers;
  out->first_cln = first_cln;
  for (int i = 0; i < layers; ++i) {
    TTS_TRY(conv_of(h, p + ".conv." + std::to_string(i), &out->conv[i]));
    if (h->cfg.multispeaker) continue;  // (conditional layer norms: their scales and shifts come from cln_weights)
    TTS_TRY(fvec(h, p + ".norm." + std::to_string(i) + ".g", &out->g[i]));
    TTS_TRY(fvec(h, p + ".norm." + std::to_string(i) + ".b", &out->b[i]));
  }
  return conv_of(h, p + ".lin", &out->lin);
}

int resolve_acoustic(Handle* h) {
  Acoustic& m = h->acoustic;
  if (m.resolved) return TTS_OK;
  TTS_TRY(conv_of(h, "embed0", &m.embed0));
  TTS_TRY(conv_of(h, "embed2", &m.embed2));
  const Dev* lang = find(h, "lang_table");
  m.lang_table = lang ? static_cast<const float*>(lang->p) : nullptr;
  for (int b = 0; b < 6; ++b) {
    TTS_TRY(block_of(h, "enc." + std::to_string(b) + ".", &m.enc[b]));
    TTS_TRY(block_of(h, "dec." + std::to_string(b) + ".", &m.dec[b]));
  }
  TTS_TRY(fvec(h, "out_norm.g", &m.out_norm_g));
  TTS_TRY(fvec(h, "out_norm.b", &m.out_norm_b));
  if (h->cfg.multispeaker) {
    TTS_TRY(conv_of(h, "hs_h", &m.hs_h));
    TTS_TRY(conv_of(h, "hs_e", &m.hs_e));
    const Dev* w;
    TTS_TRY(need(h, "cln_weights", &w));
    m.cln_weights = static_cast<const float*>(w->p);
    m.n_mlp = (int)(w->bytes / 4 / tts_cln_mlp_weight_floats(64, 256));
  }
  TTS_TRY(predictor_of(h, "pitch", 7, 0, &m.pitch));
  TTS_TRY(predictor_of(h, "energy", 2, 7, &m.energy));
  TTS_TRY(predictor_of(h, "duration", 3, 9, &m.duration));
  TTS_TRY(fvec(h, "pitch_w", &m.pitch_w));
  TTS_TRY(fvec(h, "pitch_b", &m.pitch_b));
  TTS_TRY(fvec(h, "energy_w", &m.energy_w));
  TTS_TRY(fvec(h, "energy_b", &m.energy_b));
  TTS_TRY(conv_of(h, "feat_out", &m.feat_out));
  for (int i = 0; i < 5; ++i) {
    const std::string p = "postnet." + std::to_string(i);
    TTS_TRY(conv_of(h, p + ".conv", &m.postnet[i].conv));
    TTS_TRY(fvec(h, p + ".g", &m.postnet[i].g));
    TTS_TRY(fvec(h, p + ".b", &m.postnet[i].b));
  }
  TTS_TRY(conv_of(h, "g_proj", &m.g_proj));
  for (int b = 0; b < 18; ++b) {
    const std::string p = "flow." + std::to_string(b) + ".";
    TTS_TRY(conv_of(h, p + "start", &m.flow[b].start));
    TTS_TRY(conv_of(h, p + "end", &m.flow[b].end));
    TTS_TRY(conv_of(h, p + "cond", &m.flow[b].cond));
    TTS_TRY(fvec(h, p + "winv", &m.flow[b].winv));
    TTS_TRY(fvec(h, p + "an_bias", &m.flow[b].an_bias));
    TTS_TRY(fvec(h, p + "an_logs", &m.flow[b].an_logs));
  }
  for (int g = 0; g < 5; ++g)
    for (int i = 0; i < 4; ++i) {
      const std::string p = "flowgrp." + std::to_string(g) + ".";
      TTS_TRY(conv_of(h, p + "inl." + std::to_string(i), &m.flowgrp[g].inl[i]));
      TTS_TRY(conv_of(h, p + "res_skip." + std::to_string(i), &m.flowgrp[g].res_skip[i]));
    }
  const Dev* logdet = find(h, "flow.logdet");
  m.scoring = logdet != nullptr;
  if (m.scoring) {
    TTS_CHECK_ARG(logdet->dtype == 3 && logdet->bytes == sizeof(double), "weight 'flow.logdet' is not one float64 as two int32 words of host metadata");
    memcpy(&m.flow_logdet, logdet->p, sizeof(double));
    for (int b = 0; b < 18; ++b) {
      const std::string p = "flow." + std::to_string(b) + ".";
      TTS_TRY(fvec(h, p + "wfwd", &m.flow_fwd[b].wfwd));
      TTS_TRY(conv_of(h, p + "end_ml", &m.flow_fwd[b].end_ml));
      const ConvW& e = m.flow_fwd[b].end_ml;
      TTS_CHECK_ARG(e.mode == TTS_MODE_LINEAR && e.cin == ATT && e.cout == 160 && e.taps == 1, "weight '%send_ml' is not a plain 1-tap 192 -> 160 conv", p.c_str());
    }
  }
  m.resolved = true;
  return TTS_OK;
}

int resolve_vocoder(Handle* h) {
  Vocoder& m = h->vocoder;
  if (m.resolved) return TTS_OK;
  const bool big = h->cfg.vocoder == 2;
  TTS_TRY(conv_of(h, "voc.pre", &m.pre));
  for (int i = 0; i < 4; ++i) {
    TTS_TRY(conv_of(h, "voc.ups." + std::to_string(i), &m.ups[i]));
    for (int j = 0; j < 3; ++j)
      for (int dd = 0; dd < 3; ++dd) {
        const std::string p = "voc.blk." + std::to_string(i) + "." + std::to_string(j) + "." + std::to_string(dd);
        auto& k = m.blk[i][j][dd];
        TTS_TRY(conv_of(h, p + ".c1", &k.c1));
        TTS_TRY(conv_of(h, p + ".c2", &k.c2));
        if (!big) continue;
        TTS_TRY(fvec(h, p + ".a1", &k.a1));
        TTS_TRY(fvec(h, p + ".b1", &k.b1));
        TTS_TRY(fvec(h, p + ".a2", &k.a2));
        TTS_TRY(fvec(h, p + ".b2", &k.b2));
      }
  }
  TTS_TRY(fvec(h, "voc.post_w", &m.post_w));
  if (big) {
    TTS_TRY(fvec(h, "voc.post_a", &m.post_a));
    TTS_TRY(fvec(h, "voc.post_b", &m.post_b));
    TTS_TRY(fvec(h, "voc.filt", &m.filt));
    const Dev* ft;
    TTS_TRY(need(h, "voc.fir_tab", &ft));
    m.fir_tab = ft->p;
  }
  m.resolved = true;
  return TTS_OK;
}

// 16-bit configuration (bf16 / fp16: 16-bit tensors between the fused kernels)?  TTS_COMPUTE_F32X3 is a 32-bit configuration in
// every respect but the dense products of its frame stages and vocoder (three fp16 MFMAs on split operands)
bool is16(const Handle* h) { return h->cfg.precision == TTS_COMPUTE_BF16 || h->cfg.precision == TTS_COMPUTE_F16; }
int bits16(const Handle* h) { return is16(h) ? 16 : 32; }
// the PostFlow runs the stand-alone cond convs (fp32 / f32x3 handles) and needs their output buffer
bool postflow_cond_buffer(const Handle* h) { return !is16(h); }

// relative position tables of both stacks for positions -(pmax-1) .. pmax-1 (Attention.py:177, PositionalEncoding.py:90-130):
// ptab[s][l][pmax - 1 + p] = linear_pos_l(pe(p)); the sinusoid table "pe" is uploaded by the host (fp32, built like the reference)
// and looked up here, not resolved with the model: it is uploaded again to grow
int ensure_ptabs(Handle* h, hipStream_t st) {
  const Dev* pe;
  TTS_TRY(need(h, "pe", &pe));
  const int rows = (int)pe->shape[0], pmax = (rows + 1) / 2;
  if (h->pmax == pmax && h->ptab[0]) return TTS_OK;
  TTS_TRY(hip_ok(hipStreamSynchronize(st), "position tables: sync"));
  for (int s = 0; s < 2; ++s) {
    if (h->ptab[s]) (void)hipFree(h->ptab[s]);
    TTS_TRY(hip_ok(hipMalloc(reinterpret_cast<void**>(&h->ptab[s]), (size_t)6 * rows * ATT * sizeof(float)), "position tables: hipMalloc"));
  }
  int one = rows;
  const Layout l = Layout::make(&one, 1, 1);
  for (int s = 0; s < 2; ++s)
    for (int b = 0; b < 6; ++b) {
      ConvOpt o;
      o.fp32_only = true;
      o.no_split_k = true;
      TTS_TRY(conv(h, (s ? h->acoustic.dec : h->acoustic.enc)[b].pos, T2(pe->p, ATT), T2(h->ptab[s] + (size_t)b * rows * ATT, ATT), l, st, o));
    }
  h->pmax = pmax;
  return TTS_OK;
}

// One feed-forward module in one launch (tts_ffn_fused): x <- [LN_post](x + 0.5 FFN(LN(x)))
int ffn_fused(Handle* h, const Dev* fused, const ConvW& w1, const ConvW& w2, const float* g, const float* b, const float* post_g, const float* post_b,
              float* x, int R, hipStream_t st) {
  TtsFfnDesc d;
  memset(&d, 0, sizeof(d));
  d.x = x; d.ldx = ATT; d.y = x; d.ldy = ATT; d.rows = R; d.channels = ATT;
  d.ln_g = g; d.ln_b = b;
  d.w = fused->p; d.b2 = w2.bias;
  d.post_g = post_g; d.post_b = post_b;
  d.hidden = (int)(fused->bytes / (28 * 1024)) * 32;
  d.compute = w1.compute16; d.alpha = 0.5f; d.eps = 1e-12f;
  return prof_launch(h, d.compute == TTS_COMPUTE_F16 ? "ffn_fused_f16" : "ffn_fused_bf16", 4.0 * R * ATT * d.hidden,
                     (double)R * ATT * 8 + (double)fused->bytes, (double)R * ATT, st, [&] { return tts_ffn_fused(&d, st); });
}

// norm_mha + the q | k | v projection in one launch (ln_linear, conformer_conv.hip): the bits of tts_layernorm + tts_conv1d
int ln_qkv(Handle* h, const Block& b, const float* x, float* qkv, const Layout& l, const TileTab& t128, hipStream_t st) {
  LnLinear d;
  memset(&d, 0, sizeof(d));
  d.x = x; d.ld_x = ATT; d.y = qkv; d.ld_y = 3 * ATT;
  d.ln_g = b.ln_g[1]; d.ln_b = b.ln_b[1]; d.eps = 1e-12f;
  d.w = b.qkv.w16; d.w_n = b.qkv.wn; d.bias = b.qkv.bias; d.cout = b.qkv.cout;
  d.tiles = t128.dev; d.n_tiles = t128.n; d.tile_rows = 128;
  d.compute = b.qkv.compute16;
  double rows = 0;
  for (int n : l.lengths) rows += n;
  return prof_launch(h, d.compute == TTS_COMPUTE_F16 ? "ln_qkv_f16" : "ln_qkv_bf16", 2.0 * rows * ATT * d.cout,
                     rows * (ATT + d.cout) * 4 + 2.0 * ATT * d.cout, rows * d.cout, st, [&] { return ln_linear(d, st); });
}

// The convolution module in one launch (conformer_conv.hip): x <- x2 + pw2(swish(dwconv_bn(glu(pw1(LN(x2))))))
int conv_module(Handle* h, const Block& b, int kernel, const float* x2, float* x, const Layout& l, const TileTab& tcc, hipStream_t st) {
  ConformerConv d;
  memset(&d, 0, sizeof(d));
  d.x = x2; d.ld_x = ATT; d.y = x; d.ld_y = ATT;
  d.ln_g = b.ln_g[2]; d.ln_b = b.ln_b[2]; d.eps = 1e-12f;
  d.w1 = b.pw1.w16; d.w1_n = b.pw1.wn; d.w1_half = b.pw1.half_pad; d.b1 = b.pw1.bias;
  d.dw_w = b.dw_w; d.dw_b = b.dw_b; d.kernel = kernel;
  d.w2 = b.pw2.w16; d.w2_n = b.pw2.wn; d.b2 = b.pw2.bias;
  d.tiles = tcc.dev; d.n_tiles = tcc.n; d.tile_rows = conformer_conv_tile_rows(kernel);
  d.compute = b.pw1.compute16;
  double rows = 0;
  for (int n : l.lengths) rows += n;
  return prof_launch(h, d.compute == TTS_COMPUTE_F16 ? "conformer_conv_f16" : "conformer_conv_bf16", 2.0 * rows * ATT * (3 * ATT + kernel),
                     rows * ATT * 8 + 2.0 * 3 * ATT * ATT, rows * ATT, st, [&] { return conformer_conv(d, st); });
}

// Which stacks run the fused launches (16-bit configurations; [0] encoder, [1] decoder).  The bits are the same either way: a speed
// choice per stack, never per batch or row count.  The decoder (31 taps, 640-frame utterances: seven 98-row tiles each) gains from
// both; the encoder (128-phoneme utterances: 2 x 32 workgroups on 256 CUs, each one a 128-row chain) measured SLOWER fused -
// + 0.08 ms per pass for either part - so it keeps the stand-alone launches.
constexpr bool FUSE_LN_QKV[2] = {false, true};
constexpr bool FUSE_CONV_MODULE[2] = {false, true};

// Layers/EncoderLayer.py:62-144 x 6 on the residual stream x [rows, 192] (already scaled by sqrt(192))
int conformer(Handle* h, int stack, float* x, const Layout& l, Arena& a, hipStream_t st) {
  const int R = l.total, kernel = stack ? 31 : 7;
  if (l.max_len > h->pmax) {
    set_error("conformer: %d positions exceed the uploaded position table (pmax %d): upload a larger 'pe'", l.max_len, h->pmax);
    return TTS_E_ARG;
  }
  const int b16 = bits16(h);
  TTS_ALLOC(ln, a, float, (size_t)R * ATT);
  TTS_ALLOC(hid, a, char, (size_t)R * 1536 * (b16 / 8));
  TTS_ALLOC(qkv, a, float, (size_t)R * 3 * ATT);
  TTS_ALLOC(ctx, a, float, (size_t)R * ATT);
  TTS_ALLOC(glu, a, float, (size_t)R * ATT);
  TTS_ALLOC(dwo, a, float, (size_t)R * ATT);
  TileTab t128, t64, tcc;
  TTS_TRY(tiles_of(h, l, 128, st, &t128));
  TTS_TRY(tiles_of(h, l, 64, st, &t64));
  const int fuse_mask = (FUSE_LN_QKV[stack] ? 1 : 0) | (FUSE_CONV_MODULE[stack] ? 2 : 0);
  if (b16 == 16 && (fuse_mask & 2)) TTS_TRY(tiles_of(h, l, conformer_conv_tile_rows(kernel), st, &tcc));  // (98 rows at 31 taps)
  // a packed 1-tap 192 -> n conv the fused kernels can read: the handle's 16-bit format, with a bias
  auto fusable = [&](const ConvW& c, int mode, int cout) {
    return c.w16 && c.bias && c.compute16 == h->cfg.precision && c.mode == mode && c.taps == 1 && c.cin == ATT && c.cin_pad == ATT && c.cout == cout;
  };
  const size_t prow = (size_t)(2 * h->pmax - 1) * ATT;
  for (int bi = 0; bi < 6; ++bi) {
    const Block& b = (stack ? h->acoustic.dec : h->acoustic.enc)[bi];
    ConvOpt relu, half, res1;
    relu.act = TTS_ACT_RELU;
    half.alpha = 0.5f; half.res = T2(x, ATT);
    res1.res = T2(x, ATT);
    // Macaron feed-forward (EncoderLayer.py:84-90)
    // (the same decision as engine.py: 16-bit configuration and packed weights loaded - not the number of rows: an utterance's
    // result must not depend on the batch it is in)
    const bool fuse_ffn = b16 == 16;
    if (fuse_ffn && b.ffm_fused) {
      TTS_TRY(ffn_fused(h, b.ffm_fused, b.ffm1, b.ffm2, b.ln_g[0], b.ln_b[0], nullptr, nullptr, x, R, st));
    } else {
      TTS_TRY(tts_layernorm(x, ATT, ln, ATT, b.ln_g[0], b.ln_b[0], R, ATT, 1e-12f, st));
      TTS_TRY(conv(h, b.ffm1, T2(ln, ATT), T2(hid, 1536, b16), l, st, relu));
      TTS_TRY(conv(h, b.ffm2, T2(hid, 1536, b16), T2(x, ATT), l, st, half));
    }
    // relative-position self-attention (:93-116)
    // (16-bit configurations: norm_mha inside the projection, and the convolution module as one launch - native only, same bits)
    const bool fuse_qkv = b16 == 16 && (fuse_mask & 1) && fusable(b.qkv, TTS_MODE_LINEAR, 3 * ATT);
    const bool fuse_conv = b16 == 16 && (fuse_mask & 2) && fusable(b.pw1, TTS_MODE_GLU, ATT) && fusable(b.pw2, TTS_MODE_LINEAR, ATT);
    if (fuse_qkv) {
      TTS_TRY(ln_qkv(h, b, x, qkv, l, t128, st));
    } else {
      TTS_TRY(tts_layernorm(x, ATT, ln, ATT, b.ln_g[1], b.ln_b[1], R, ATT, 1e-12f, st));
      TTS_TRY(conv(h, b.qkv, T2(ln, ATT), T2(qkv, 3 * ATT), l, st));
    }
    if (b16 == 16)  // (16-bit configurations: the contractions on the fp16 matrix cores)
      TTS_TRY(tts_relpos_attention_f16(qkv, 3 * ATT, h->ptab[stack] + bi * prow, h->pmax, b.u, b.v, ctx, ATT, HEADS, DK, t128.dev, t128.n, 128, st));
    else
      TTS_TRY(tts_relpos_attention(qkv, 3 * ATT, h->ptab[stack] + bi * prow, h->pmax, b.u, b.v, ctx, ATT, HEADS, DK, t128.dev, t128.n, 128,
                                   h->split_mode == 2 ? TTS_ATT_KEY_SPLIT_ALWAYS : (h->split_mode == 1 ? TTS_ATT_KEY_SPLIT : 0), st));
    // convolution module (:119-125, Convolution.py:31-55)
    if (fuse_conv) {
      // The fused module cannot update x in place (a workgroup reads its neighbours' rows as halo), so the out projection leaves
      // x + out(ctx) in the (otherwise unused) glu buffer and the module writes x: x keeps the bits it has today in every row,
      // the gap rows between utterances included; the buffer's gap rows are never read (halos are clamped to the utterance).
      TTS_TRY(conv(h, b.out, T2(ctx, ATT), T2(glu, ATT), l, st, res1));
      TTS_TRY(conv_module(h, b, kernel, glu, x, l, tcc, st));
    } else {
      TTS_TRY(conv(h, b.out, T2(ctx, ATT), T2(x, ATT), l, st, res1));
      TTS_TRY(tts_layernorm(x, ATT, ln, ATT, b.ln_g[2], b.ln_b[2], R, ATT, 1e-12f, st));
      TTS_TRY(conv(h, b.pw1, T2(ln, ATT), T2(glu, ATT), l, st));
      TTS_TRY(tts_dwconv_swish(glu, ATT, dwo, ATT, b.dw_w, b.dw_b, ATT, kernel, t64.dev, t64.n, 64, st));
      TTS_TRY(conv(h, b.pw2, T2(dwo, ATT), T2(x, ATT), l, st, res1));
    }
    // feed-forward (:128-133) and the block's final norm (:135-136)
    if (fuse_ffn && b.ff_fused) {  // (with the block's final norm in its epilogue)
      TTS_TRY(ffn_fused(h, b.ff_fused, b.ff1, b.ff2, b.ln_g[3], b.ln_b[3], b.ln_g[4], b.ln_b[4], x, R, st));
    } else {
      TTS_TRY(tts_layernorm(x, ATT, ln, ATT, b.ln_g[3], b.ln_b[3], R, ATT, 1e-12f, st));
      TTS_TRY(conv(h, b.ff1, T2(ln, ATT), T2(hid, 1536, b16), l, st, relu));
      TTS_TRY(conv(h, b.ff2, T2(hid, 1536, b16), T2(x, ATT), l, st, half));
      TTS_TRY(tts_layernorm(x, ATT, x, ATT, b.ln_g[4], b.ln_b[4], R, ATT, 1e-12f, st));
    }
  }
  return TTS_OK;
}

size_t conformer_bytes(size_t R) { return R * (ATT * 4 * 4 + 1536 * 4 + 3 * ATT * 4) + 8 * 256; }

// Arena sizes: ONE set of expressions for the stage entries (what they reserve) and for tts_workspace_bytes (what it promises).
size_t phone_arena_bytes(size_t R, size_t B) {
  return conformer_bytes(R) + R * (100 + 3 * ATT + 6 * 256 + 16) * 4 + B * (64 + 2 * ATT + 24 * 256 + 8) * 4 + (1 << 16) +
         2 * (B + R) * TTS_PROSODY_STATS * 4 + 256 +  // (the statistics blocks of tts_control_and_regulate_v and _c: utterances, at most R spans)
         2 * B * TTS_PROSODY_STATS * 4 + 256 +  // (once a second statistics buffer; kept, so that tts_workspace_bytes answers as it did)
         // tts_control_and_regulate_t: the written scales and curves, the extra frames, the report of at most R segments
         B * TTS_PROSODY_SCALES * 4 + R * (TTS_PROSODY_CURVE_COLUMNS + 1 + TTS_FIT_COLUMNS) * 4 + 4 * 256;
}
// cond_buffer: the PostFlow keeps the coupling blocks' conditioning [RS, 1536] in memory (every configuration but the 16-bit ones
// with the fused WaveNet layer, which computes it inside the layer).  Those configurations run a coupling block as one launch: the
// [hidden state | skip sum] buffer ([RF / 2, 384]) is not allocated, a second x ([RF / 2, 160]) is: ATT - 80 floats per frame less.
size_t frame_arena_bytes(size_t RF, bool cond_buffer) {
  return conformer_bytes(RF) +
         RF * ((80 + ATT) + 2 * ATT + 3 * 80 + 2 * 256 + ATT + 160 + 4 * ATT + ATT + (cond_buffer ? 8 * ATT : 0) - (cond_buffer ? 0 : ATT - 80) + 64) * 4 + (64 << 20);
}
// vocoder: R packed mel rows.  Arena 1 holds the pre-conv output [R, 512] fp32 and later the stages 1 and 3, arena 0 the stages 0 and 2
// (a stage reads its input from the other arena).  Per stage: the up-sampled tensor, the stage output and two ping-pong buffers of
// [rows, channels] - plus, where the residual steps are not fused (fp32 configuration; 256 channels), the conv intermediate and
// for BigVGAN the two stand-alone snake outputs.  16-bit configurations keep 16-bit stage tensors.
size_t vocoder_stage_bytes(size_t R, int stage, bool fused_mode, bool big) {
  static const int UPS[4] = {8, 48, 192, 384};
  const size_t ch = 256 >> stage, rows = R * UPS[stage], se = fused_mode ? 2 : 4;
  const bool fused = fused_mode && ch <= 128;
  const size_t tensors = 4 + (fused ? 0 : (big ? 3 : 1));
  return tensors * (((rows * ch * se) + 255) & ~(size_t)255) + (1 << 20);
}
size_t vocoder_arena_bytes(size_t R, int arena, bool fused_mode, bool big) {
  size_t m = arena == 1 ? R * 512 * 4 + (1 << 20) : 0;
  for (int i = arena; i < 4; i += 2) m = std::max(m, vocoder_stage_bytes(R, i, fused_mode, big));
  return m;
}
size_t with_growth_slack(size_t bytes) { return bytes + bytes / 8 + (1 << 20); }  // what arena_reserve allocates for a request

int predictor(Handle* h, const Predictor& p, float* out, hipStream_t st) {
  const Layout& l = h->lp;
  const int R = l.total;
  TTS_ALLOC(a, h->phone, float, (size_t)R * 256);
  TTS_ALLOC(bb, h->phone, float, (size_t)R * 256);
  TileTab t64;
  TTS_TRY(tiles_of(h, l, 64, st, &t64));
  const float* cur = h->enc;
  int ld = ATT;
  for (int i = 0; i < p.layers; ++i) {
    ConvOpt o;
    o.act = TTS_ACT_RELU;
    o.fp32_only = true;
    TTS_TRY(conv(h, p.conv[i], T2(const_cast<float*>(cur), ld), T2(a, 256), l, st, o));
    if (h->cfg.multispeaker) {
      const float* sc = h->cln + (size_t)(2 * (p.first_cln + i)) * h->B * 256;
      TTS_TRY(tts_cond_layernorm(a, 256, bb, 256, sc, sc + (size_t)h->B * 256, 256, t64.dev, t64.n, 64, st));
    } else {
      TTS_TRY(tts_layernorm(a, 256, bb, 256, p.g[i], p.b[i], R, 256, 1e-12f, st));
    }
    cur = bb;
    ld = 256;
  }
  ConvOpt o;
  o.fp32_only = true;
  return conv(h, p.lin, T2(const_cast<float*>(cur), ld), T2(out, 1), l, st, o);
}

}  // namespace

// ======================================================================================================================
int pipeline_create(const TtsConfig* cfg, Handle** out) {
  TTS_CHECK_ARG(cfg && out, "tts_create: null pointer");
  TTS_CHECK_ARG(cfg->precision >= 0 && cfg->precision <= 3, "tts_create: precision %d (0 fp32, 1 bf16, 2 fp16, 3 split fp32)", cfg->precision);
  TTS_CHECK_ARG(cfg->vocoder >= 0 && cfg->vocoder <= 2, "tts_create: vocoder %d (0 none, 1 hifigan, 2 bigvgan)", cfg->vocoder);
  Handle* h = new Handle();
  h->cfg = *cfg;
  if (cfg->small_tile_blocks > 0) h->small_tile_blocks = cfg->small_tile_blocks;
  *out = h;
  return TTS_OK;
}

int pipeline_destroy(Handle* h) {
  if (!h) return TTS_OK;
  (void)hipDeviceSynchronize();
  for (auto& kv : h->weights)
    if (kv.second.dtype != 3 && kv.second.p) (void)hipFree(kv.second.p);
    else free(kv.second.p);
  for (auto& group : h->tabs)
    for (TableStore& s : group) {
      for (TableChunk& c : s.chunks) {
        (void)hipFree(c.dev);
        (void)hipHostFree(c.host);
      }
      if (s.last_use) (void)hipEventDestroy(s.last_use);
    }
  for (Arena* a : {&h->phone, &h->frame, &h->voc[0], &h->voc[1], &h->nll})
    if (a->base) (void)hipFree(a->base);
  for (int s = 0; s < 2; ++s)
    if (h->ptab[s]) (void)hipFree(h->ptab[s]);
  delete h;
  return TTS_OK;
}

int pipeline_load(Handle* h, const char* name, const void* host, const int64_t* shape, int ndim, int dtype) {
  TTS_CHECK_ARG(h && name && host && shape, "tts_load_weights: null pointer");
  TTS_CHECK_ARG(ndim >= 1 && ndim <= 4, "tts_load_weights(%s): ndim %d", name, ndim);
  TTS_CHECK_ARG(dtype >= 0 && dtype <= 4, "tts_load_weights(%s): dtype %d (0 f32, 1 bf16, 2 f16, 3 i32 host metadata, 4 u8)", name, dtype);
  static const int esz[5] = {4, 2, 2, 4, 1};
  Dev d;
  d.ndim = ndim;
  d.dtype = dtype;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    d.shape[i] = shape[i];
    n *= (size_t)shape[i];
  }
  d.bytes = n * esz[dtype];
  h->acoustic.resolved = h->vocoder.resolved = false;  // (a replaced tensor frees what the model points to: the next pass resolves again)
  auto it = h->weights.find(name);
  if (it != h->weights.end()) {  // replacing a tensor (e.g. a longer position table): nothing may still read the old one
    (void)hipDeviceSynchronize();
    if (it->second.dtype == 3) free(it->second.p);
    else (void)hipFree(it->second.p);
    h->weights.erase(it);
    if (!strcmp(name, "pe")) h->pmax = 0;
  }
  if (dtype == 3) {  // descriptor fields: read by the host sequencer only
    d.p = malloc(std::max<size_t>(d.bytes, 4));
    memcpy(d.p, host, d.bytes);
  } else {
    TTS_TRY(hip_ok(hipMalloc(&d.p, std::max<size_t>(d.bytes, 256)), "tts_load_weights: hipMalloc"));
    TTS_TRY(hip_ok(hipMemcpy(d.p, host, d.bytes, hipMemcpyHostToDevice), "tts_load_weights: upload"));
  }
  h->weights[name] = d;
  return TTS_OK;
}

// upper bound of the workspace a batch of B utterances with at most Lmax phonemes / Tmax frames each will claim: the sum of what the
// stage entries reserve for such a batch (same expressions), arena growth slack included (tts_workspace_claimed reports the real sum)
long long pipeline_workspace_bytes(const Handle* h, int B, int Lmax, int Tmax) {
  if (!h || B <= 0) return 0;
  const size_t RP = (size_t)B * Lmax, RF = (size_t)B * (Tmax + 1);  // (frame layouts start every utterance on an even row)
  size_t total = with_growth_slack(phone_arena_bytes(RP, B)) + with_growth_slack(frame_arena_bytes(RF, postflow_cond_buffer(h)));
  if (h->cfg.vocoder) {
    const bool fused_mode = is16(h), big = h->cfg.vocoder == 2;
    for (int a = 0; a < 2; ++a) total += with_growth_slack(vocoder_arena_bytes(RF, a, fused_mode, big));
  }
  return (long long)total;
}

long long pipeline_workspace_claimed(const Handle* h) {
  if (!h) return 0;
  return (long long)(h->phone.cap + h->frame.cap + h->voc[0].cap + h->voc[1].cap + h->nll.cap);
}

// ---- stage A.1: encoder ----------------------------------------------------------------------------------------------
int pipeline_encoder(Handle* h, const float* text, const float* utt_emb, const int* lang_ids, const int* phone_lengths, int B,
                     hipStream_t st) {
  TTS_CHECK_ARG(h && text && phone_lengths && B > 0, "tts_encoder: bad arguments");
  TTS_CHECK_ARG(!h->cfg.multispeaker || utt_emb, "tts_encoder: the multi-speaker checkpoint needs utterance embeddings");
  TTS_TRY(resolve_acoustic(h));  // (a missing tensor of any acoustic stage: reported before anything is reserved or enqueued)
  const Acoustic& m = h->acoustic;
  h->split_mode = 2;
  TTS_TRY(tables_begin(h, 0, st));  // a batch starts: its tile tables go to the acoustic stages' other generation
  h->lp = Layout::make(phone_lengths, B, 1);
  h->B = B;
  h->text = text;
  h->have_flow = false;
  h->pstats = nullptr;
  h->pstats_host.clear();
  h->n_spans = -1;
  h->sstats_host.clear();
  h->fit_ws = nullptr;
  h->n_fit = -1;
  h->fit_host.clear();
  h->fit_extra_host.clear();
  const int R = h->lp.total;
  TTS_TRY(arena_reserve(h->phone, phone_arena_bytes(R, B), st));
  TTS_TRY(ensure_ptabs(h, st));
  Arena& a = h->phone;
  int bn = B;
  const Layout lb = Layout::make(&bn, 1, 1);
  TTS_ALLOC(e_norm, a, float, (size_t)B * 64);
  h->e_norm = e_norm;
  if (utt_emb) TTS_TRY(tts_l2_normalize(utt_emb, e_norm, B, 64, st));
  TTS_ALLOC(h100, a, float, (size_t)R * 100);
  ConvOpt o0;
  o0.act = TTS_ACT_TANH;
  o0.fp32_only = true;
  TTS_TRY(conv(h, m.embed0, T2(const_cast<float*>(text), 62), T2(h100, 100), h->lp, st, o0));
  ConvOpt o2;
  o2.alpha = sqrtf((float)ATT);
  o2.fp32_only = true;
  if (h->cfg.multilingual && lang_ids) {  // Conformer.py:112-114
    if (!m.lang_table) {
      set_error("weight '%s' was not loaded (tts_load_weights)", "lang_table");
      return TTS_E_ARG;
    }
    TTS_ALLOC(lang, a, float, (size_t)B * ATT);
    TTS_TRY(tts_gather_rows(m.lang_table, ATT, lang_ids, lang, ATT, B, ATT, st));
    o2.seqvec = lang;
    o2.ld_seqvec = ATT;
  }
  TTS_ALLOC(x, a, float, (size_t)R * ATT);
  TTS_TRY(conv(h, m.embed2, T2(h100, 100), T2(x, ATT), h->lp, st, o2));
  TTS_TRY(conformer(h, 0, x, h->lp, a, st));
  TTS_TRY(tts_layernorm(x, ATT, x, ATT, m.out_norm_g, m.out_norm_b, R, ATT, 1e-12f, st));
  if (h->cfg.multispeaker) {  // Conformer.py:130-134: projection of [hidden | normalised utterance embedding]
    TTS_ALLOC(e_proj, a, float, (size_t)B * ATT);
    ConvOpt oe;
    oe.fp32_only = true;
    TTS_TRY(conv(h, m.hs_e, T2(e_norm, 64), T2(e_proj, ATT), lb, st, oe));
    TTS_ALLOC(enc, a, float, (size_t)R * ATT);
    ConvOpt oh;
    oh.seqvec = e_proj;
    oh.ld_seqvec = ATT;
    TTS_TRY(conv(h, m.hs_h, T2(x, ATT), T2(enc, ATT), h->lp, st, oh));
    h->enc = enc;
  } else {
    h->enc = x;
  }
  TTS_ALLOC(p, a, float, R);
  TTS_ALLOC(e, a, float, R);
  TTS_ALLOC(dd, a, int, R);
  h->pitch = p; h->energy = e; h->dur = dd;
  h->cln = nullptr;
  return TTS_OK;
}

// the scales and shifts of the predictors' conditional layer norms from the utterance embedding (multi-speaker checkpoints)
int cln_prepare(Handle* h, hipStream_t st) {
  const Acoustic& m = h->acoustic;
  TTS_ALLOC(cln, h->phone, float, (size_t)m.n_mlp * h->B * 256);
  TTS_TRY(tts_cln_mlp(h->e_norm, h->B, 64, 256, m.cln_weights, m.n_mlp, cln, st));
  h->cln = cln;
  return TTS_OK;
}

// ---- stage A.2: pitch / energy / duration predictors (gold values replace a prediction) --------------------------------
int pipeline_predictors(Handle* h, const float* gold_pitch, const float* gold_energy, const int* gold_dur, hipStream_t st) {
  TTS_CHECK_ARG(h && h->enc, "tts_variance_predictors: run tts_encoder first");
  TTS_CHECK_RESOLVED(h, "tts_variance_predictors");
  h->split_mode = 2;
  h->tab_which = 0;
  const Acoustic& m = h->acoustic;
  const int R = h->lp.total;
  if (h->cfg.multispeaker && !(gold_pitch && gold_energy && gold_dur)) TTS_TRY(cln_prepare(h, st));
  if (gold_pitch) TTS_TRY(hip_ok(hipMemcpyAsync(h->pitch, gold_pitch, (size_t)R * 4, hipMemcpyDeviceToDevice, st), "gold pitch"));
  else TTS_TRY(predictor(h, m.pitch, h->pitch, st));
  if (gold_energy) TTS_TRY(hip_ok(hipMemcpyAsync(h->energy, gold_energy, (size_t)R * 4, hipMemcpyDeviceToDevice, st), "gold energy"));
  else TTS_TRY(predictor(h, m.energy, h->energy, st));
  if (gold_dur) {
    TTS_TRY(hip_ok(hipMemcpyAsync(h->dur, gold_dur, (size_t)R * 4, hipMemcpyDeviceToDevice, st), "gold durations"));
  } else {
    TTS_ALLOC(logd, h->phone, float, R);
    TTS_TRY(predictor(h, m.duration, logd, st));
    TTS_TRY(tts_duration_from_log(logd, h->dur, R, st));
  }
  return TTS_OK;
}

// Per-utterance frame counts from the durations in dur_dev (the one host round trip of a pass), then the frame layout, its arena and
// the length regulator (LengthRegulator.py:37-61) on h->dur.  gold (teacher forcing): the durations are the caller's, so negative
// ones and oversized totals are argument errors, and the embeddings are added in the training order - tts_length_regulate forms
// enc + (first * w1 + b1) + (second * w2 + b2): encoded + energy_embed + pitch_embed there, pitch first at inference.
int regulate(Handle* h, const int* dur_dev, bool gold, int* frames_out, hipStream_t st) {
  const Acoustic& m = h->acoustic;
  const int R = h->lp.total, B = h->B;
  const int *pb, *pe;
  TTS_TRY(bounds_of(h, h->lp, st, &pb, &pe));
  std::vector<int> d_host(R);
  TTS_TRY(hip_ok(hipMemcpyAsync(d_host.data(), dur_dev, (size_t)R * 4, hipMemcpyDeviceToHost, st), "durations to host"));
  TTS_TRY(hip_ok(hipStreamSynchronize(st), "durations to host: sync"));
  h->frames.assign(B, 0);
  for (int u = 0; u < B; ++u) {
    long long t = 0;
    for (int i = 0; i < h->lp.lengths[u]; ++i) {
      const int d = d_host[h->lp.begins[u] + i];
      TTS_CHECK_ARG(!gold || d >= 0, "tts_teacher_forced: utterance %d, phoneme %d: negative gold duration %d", u, i, d);
      t += d;
    }
    TTS_CHECK_ARG(!gold || t <= (1 << 24), "tts_teacher_forced: utterance %d: %lld frames", u, t);
    h->frames[u] = t > 0 ? (int)t : h->lp.lengths[u];  // LengthRegulator.py:52-53: an all-zero utterance becomes all ones
    if (frames_out) frames_out[u] = h->frames[u];
  }
  h->lf = Layout::make(h->frames.data(), B, 2);  // even begins: the Glow squeeze is a pure re-view
  const size_t RF = h->lf.total;
  TTS_TRY(arena_reserve(h->frame, frame_arena_bytes(RF, postflow_cond_buffer(h)), st));
  Arena& a = h->frame;
  TTS_ALLOC(cat, a, float, RF * (80 + ATT));  // [refined mel | up-sampled text] = g_proj input
  TTS_TRY(hip_ok(hipMemsetAsync(cat, 0, RF * (80 + ATT) * 4, st), "clear frame buffer"));
  TTS_ALLOC(dec, a, float, RF * ATT);
  h->cat = cat;
  h->dec = dec;
  const int *fb, *fe;
  TTS_TRY(bounds_of(h, h->lf, st, &fb, &fe));
  if (gold)
    return tts_length_regulate(h->enc, ATT, h->energy, h->pitch, m.energy_w, m.energy_b, m.pitch_w, m.pitch_b, h->dur, pb, pe, fb, B, h->lf.max_len,
                               h->lp.max_len, ATT, cat + 80, 80 + ATT, dec, ATT, sqrtf((float)ATT), st);
  return tts_length_regulate(h->enc, ATT, h->pitch, h->energy, m.pitch_w, m.pitch_b, m.energy_w, m.energy_b, h->dur, pb, pe, fb, B, h->lf.max_len,
                             h->lp.max_len, ATT, cat + 80, 80 + ATT, dec, ATT, sqrtf((float)ATT), st);
}

// ---- stage A.3 / B.0: control, the one host round trip, length regulator -----------------------------------------------
// What one of the three entries asks for (include/toucan_tts.h, toucan_prosody.h, toucan_prosody_curves.h).
struct ControlRequest {
  const char* entry;                      // its name, for messages
  enum { BATCH, UTTERANCE, PHONEME, FIT } kind;  // the scalar, the _v, the _c, the _t entry; the last three take the statistics
  float batch[4] = {1.f, 1.f, 1.f, 1.f};  // the scalar entry's scales: duration, pitch variance, energy variance, pause
  const float* scales = nullptr;          // host [B][4]: UTTERANCE, and optional with PHONEME and FIT
  const float* curves = nullptr;          // host [R][5]: PHONEME, and optional with FIT
  const int* spans = nullptr;             // host [n_spans][2] packed row ranges, with curves only
  int n_spans = 0;
  const float* segments = nullptr;        // host [n_seg][TTS_FIT_COLUMNS]: FIT only (include/toucan_prosody_fit.h)
  int n_seg = 0;
};

// The _t entry's segment table against the batch's layout: everything include/toucan_prosody_fit.h asks of it.
int check_fit_segments(const char* entry, const Layout& lp, const float* seg, int n_seg) {
  const int B = lp.n(), R = lp.total;
  TTS_CHECK_ARG(seg && n_seg >= 1, "%s: %d segments and %s segment table (a call without segments takes tts_control_and_regulate_c)", entry, n_seg,
                seg ? "a" : "no");
  TTS_CHECK_ARG(n_seg <= R, "%s: %d segments, the batch has %d phoneme rows", entry, n_seg, R);
  TTS_CHECK_ARG(R <= TTS_FIT_MAX_TARGET, "%s: %d phoneme rows, the segment table holds row numbers up to 2^24", entry, R);
  std::vector<int> whole(B, 0), parts(B, 0);
  std::vector<std::pair<int, int>> order;  // (begin, segment)
  for (int s = 0; s < n_seg; ++s) {
    const float* q = seg + (size_t)s * TTS_FIT_COLUMNS;
    for (int k = 0; k < TTS_FIT_COLUMNS; ++k) TTS_CHECK_ARG(std::isfinite(q[k]), "%s: segment %d: column %d is %g, it must be finite", entry, s, k, (double)q[k]);
    TTS_CHECK_ARG(q[0] >= 0.f && q[0] < (float)B && q[0] == std::floor(q[0]), "%s: segment %d: utterance %g, the batch has %d", entry, s, (double)q[0], B);
    const int u = (int)q[0];
    TTS_CHECK_ARG(q[1] == (float)TTS_FIT_UTT_DURATION || q[1] == (float)TTS_FIT_UTT_PAUSE || q[1] == (float)TTS_FIT_SPAN,
                  "%s: utterance %d, segment %d: kind %g is none of 0, 1, 2", entry, u, s, (double)q[1]);
    const int kind = (int)q[1], b0 = lp.begins[u], b1 = b0 + lp.lengths[u];
    TTS_CHECK_ARG(q[2] == std::floor(q[2]) && q[3] == std::floor(q[3]) && q[2] >= (float)b0 && q[2] < q[3] && q[3] <= (float)b1,
                  "%s: utterance %d, segment %d: rows [%g, %g) are empty or outside the utterance's rows [%d, %d)", entry, u, s, (double)q[2],
                  (double)q[3], b0, b1);
    TTS_CHECK_ARG(kind == TTS_FIT_SPAN || ((int)q[2] == b0 && (int)q[3] == b1), "%s: utterance %d, segment %d: kind %d takes the whole utterance", entry,
                  u, s, kind);
    TTS_CHECK_ARG(q[4] >= 1.f && q[4] <= (float)TTS_FIT_MAX_TARGET && q[4] == std::floor(q[4]),
                  "%s: utterance %d, segment %d: the target %g is no whole number of frames in 1 .. 2^24", entry, u, s, (double)q[4]);
    TTS_CHECK_ARG(q[5] <= q[6] && q[6] <= (float)TTS_FIT_MAX_BOUND && (kind == TTS_FIT_UTT_PAUSE ? q[5] >= 0.f : q[5] > 0.f),
                  "%s: utterance %d, segment %d: bounds [%g, %g] must be ordered, %s and at most %d", entry, u, s, (double)q[5], (double)q[6],
                  kind == TTS_FIT_UTT_PAUSE ? "not negative" : "positive", TTS_FIT_MAX_BOUND);
    TTS_CHECK_ARG(q[7] == 0.f || q[7] == 1.f, "%s: utterance %d, segment %d: exact is %g, not 0 or 1", entry, u, s, (double)q[7]);
    (kind == TTS_FIT_SPAN ? parts : whole)[u] += 1;
    TTS_CHECK_ARG(whole[u] <= 1 && !(whole[u] && parts[u]), "%s: utterance %d, segment %d: a whole-utterance segment stands alone in its utterance", entry,
                  u, s);
    order.emplace_back((int)q[2], s);
  }
  std::sort(order.begin(), order.end());
  for (size_t i = 1; i < order.size(); ++i) {
    const float* p = seg + (size_t)order[i - 1].second * TTS_FIT_COLUMNS;
    TTS_CHECK_ARG((int)p[3] <= order[i].first, "%s: utterance %d: segments %d and %d overlap", entry, (int)p[0], order[i - 1].second, order[i].second);
  }
  return TTS_OK;
}

// A host array goes up through the table store of the acoustic stages under the key name + bytes (pinned staging, one asynchronous
// copy on st).  The store already orders the reuse of its staging behind the last use of a generation, and a table that repeats -
// an emphasis sweep run twice, a server's handful of presets - is found there, not uploaded; one that never repeats costs its bytes
// once in the store and once in the key until the generation passes TABLE_BUDGET and is rewound.  (A layout key is 4 (2 n + 1)
// bytes of begins and lengths, these start with a name: the two kinds never collide.)
template <class T>
int table_named(Handle* h, const char* name, const T* host, size_t n, hipStream_t st, const T** dev) {
  std::string key(name);
  key.append(reinterpret_cast<const char*>(host), n * sizeof(T));
  void* d;
  TTS_TRY(table_of(h, key, st, [&] { return std::vector<T>(host, host + n); }, &d, nullptr));
  *dev = static_cast<const T*>(d);
  return TTS_OK;
}

// Scalar entry: one control launch, then regulate().  Per-utterance entries: overrides -> statistics (utterances, spans) -> scales
// and curves -> statistics (utterances, spans), then regulate(): its duration read-back is the one host round trip, and the
// statistics ride on it (their copies are enqueued in front of it).  With segments the solver runs between the first statistics and
// the control launch, which then reads the tables the solver wrote, and the repair's extra frames are added behind it; the report,
// the solved scales and the extra frames ride on the same round trip.  Nothing is enqueued before every value has been checked.
int control_regulate(Handle* h, const ControlRequest& q, int* frames_out, hipStream_t st) {
  TTS_CHECK_ARG(h && h->enc && h->dur, "%s: run tts_encoder and tts_variance_predictors first", q.entry);
  const int B = h->B, R = h->lp.total, n_spans = q.n_spans;
  if (q.kind == ControlRequest::BATCH) TTS_CHECK_ARG(q.batch[0] > 0.f, "%s: duration_scaling_factor must be positive", q.entry);
  if (q.kind == ControlRequest::UTTERANCE) TTS_CHECK_ARG(q.scales, "%s: null scales", q.entry);
  if (q.kind == ControlRequest::PHONEME) {
    TTS_CHECK_ARG(q.curves, "%s: null curves", q.entry);
    TTS_CHECK_ARG(n_spans >= 0 && (q.spans || n_spans == 0), "%s: %d spans and %s span table", q.entry, n_spans, q.spans ? "a" : "no");
    TTS_CHECK_ARG(n_spans <= R, "%s: %d spans, the entry takes at most one per phoneme row (%d)", q.entry, n_spans, R);
  }
  const bool fit = q.kind == ControlRequest::FIT;
  bool fit_spans = false;
  if (fit) {
    TTS_CHECK_ARG(n_spans >= 0 && (q.spans || n_spans == 0) && (q.curves || n_spans == 0), "%s: %d spans need a span table and a curve table", q.entry,
                  n_spans);
    TTS_CHECK_ARG(n_spans <= R, "%s: %d spans, the entry takes at most one per phoneme row (%d)", q.entry, n_spans, R);
    TTS_TRY(check_fit_segments(q.entry, h->lp, q.segments, q.n_seg));
    for (int s = 0; s < q.n_seg; ++s) fit_spans |= q.segments[(size_t)s * TTS_FIT_COLUMNS + 1] == (float)TTS_FIT_SPAN;
  }
  for (int u = 0; u < B; ++u) {
    if (q.scales) {
      const float ds = q.scales[(size_t)u * TTS_PROSODY_SCALES];
      TTS_CHECK_ARG(std::isfinite(ds) && ds > 0.f, "%s: utterance %d: duration_scaling_factor %g must be positive and finite", q.entry, u, (double)ds);
    }
    for (int i = 0; q.curves && i < h->lp.lengths[u]; ++i) {
      const float* c = q.curves + (size_t)(h->lp.begins[u] + i) * TTS_PROSODY_CURVE_COLUMNS;
      TTS_CHECK_ARG(std::isfinite(c[0]) && c[0] > 0.f, "%s: utterance %d, phoneme %d: duration factor %g must be positive and finite", q.entry, u, i,
                    (double)c[0]);
      for (int k = 1; k < TTS_PROSODY_CURVE_COLUMNS; ++k)
        TTS_CHECK_ARG(std::isfinite(c[k]), "%s: utterance %d, phoneme %d: curve column %d is %g, it must be finite", q.entry, u, i, k, (double)c[k]);
    }
  }
  for (int s = 0; s < n_spans; ++s)
    TTS_CHECK_ARG(0 <= q.spans[2 * s] && q.spans[2 * s] <= q.spans[2 * s + 1] && q.spans[2 * s + 1] <= R, "%s: span %d is rows [%d, %d), the batch has %d",
                  q.entry, s, q.spans[2 * s], q.spans[2 * s + 1], R);
  TTS_CHECK_RESOLVED(h, q.entry);
  h->tab_which = 0;
  const int *pb, *pe;
  TTS_TRY(bounds_of(h, h->lp, st, &pb, &pe));
  if (q.kind == ControlRequest::BATCH) {
    TTS_TRY(tts_prosody_control(h->text, 62, h->pitch, h->energy, h->dur, pb, pe, B, q.batch[0], q.batch[1], q.batch[2], q.batch[3], st));
    return regulate(h, h->dur, false, frames_out, st);
  }
  const float *sdev = nullptr, *cdev = nullptr;
  const int *xb = nullptr, *xe = nullptr;
  if (q.scales) TTS_TRY(table_named(h, "prosody_scales", q.scales, (size_t)B * TTS_PROSODY_SCALES, st, &sdev));
  if (q.curves) TTS_TRY(table_named(h, "prosody_curves", q.curves, (size_t)R * TTS_PROSODY_CURVE_COLUMNS, st, &cdev));
  if (n_spans > 0) {  // (begin[n_spans] | end[n_spans]), the form tts_prosody_stats takes
    std::vector<int> bounds(2 * (size_t)n_spans);
    for (int s = 0; s < n_spans; ++s) {
      bounds[s] = q.spans[2 * s];
      bounds[n_spans + s] = q.spans[2 * s + 1];
    }
    TTS_TRY(table_named(h, "prosody_spans", bounds.data(), bounds.size(), st, &xb));
    xe = xb + n_spans;
  }
  const size_t NU = (size_t)B * TTS_PROSODY_STATS, NX = (size_t)n_spans * TTS_PROSODY_STATS;
  if (!h->pstats) {
    TTS_ALLOC(ps, h->phone, float, 2 * (size_t)(B + R) * TTS_PROSODY_STATS);
    h->pstats = ps;
  }
  float *ubefore = h->pstats, *uafter = ubefore + NU, *xbefore = uafter + NU, *xafter = xbefore + NX;
  const int n_seg = q.n_seg;
  const int *gb = nullptr, *ge = nullptr, *gu = nullptr, *gk = nullptr;
  const float* gspec = nullptr;
  float *fit_scales = nullptr, *fit_curves = nullptr, *fit_report = nullptr;
  int* fit_extra = nullptr;
  if (fit) {  // the segment table as the kernel takes it: (begin | end | utterance | kind)[n_seg] and [n_seg][target, lo, hi, exact]
    std::vector<int> ints(4 * (size_t)n_seg);
    std::vector<float> spec((size_t)n_seg * TTS_FIT_SPEC);
    for (int s = 0; s < n_seg; ++s) {
      const float* g = q.segments + (size_t)s * TTS_FIT_COLUMNS;
      ints[s] = (int)g[2];
      ints[n_seg + s] = (int)g[3];
      ints[2 * (size_t)n_seg + s] = (int)g[0];
      ints[3 * (size_t)n_seg + s] = (int)g[1];
      for (int k = 0; k < TTS_FIT_SPEC; ++k) spec[(size_t)s * TTS_FIT_SPEC + k] = g[4 + k];
    }
    TTS_TRY(table_named(h, "prosody_fit_rows", ints.data(), ints.size(), st, &gb));
    TTS_TRY(table_named(h, "prosody_fit_spec", spec.data(), spec.size(), st, &gspec));
    ge = gb + n_seg; gu = ge + n_seg; gk = gu + n_seg;
    if (!h->fit_ws) {
      TTS_ALLOC(ws, h->phone, float, (size_t)B * TTS_PROSODY_SCALES + (size_t)R * (TTS_PROSODY_CURVE_COLUMNS + TTS_FIT_COLUMNS + 1));
      h->fit_ws = ws;
    }
    fit_scales = h->fit_ws;
    fit_curves = fit_scales + (size_t)B * TTS_PROSODY_SCALES;
    fit_report = fit_curves + (size_t)R * TTS_PROSODY_CURVE_COLUMNS;
    fit_extra = reinterpret_cast<int*>(fit_report + (size_t)R * TTS_FIT_COLUMNS);
    if (!q.curves && !fit_spans) fit_curves = nullptr;
  }
  TTS_TRY(tts_prosody_control_v(h->text, 62, h->pitch, h->energy, h->dur, pb, pe, B, nullptr, st));
  TTS_TRY(tts_prosody_stats(h->pitch, h->energy, h->dur, pb, pe, B, ubefore, st));
  TTS_TRY(tts_prosody_stats(h->pitch, h->energy, h->dur, xb, xe, n_spans, xbefore, st));  // (no spans: no launch)
  if (fit) {  // the solver writes tables of its own in the workspace: those of the table store are shared between batches
    TTS_TRY(tts_prosody_fit(h->text, 62, h->dur, pb, pe, B, gb, ge, gu, gk, n_seg, gspec, sdev, cdev, fit_scales, fit_curves, fit_extra, fit_report, st));
    if (fit_curves) TTS_TRY(tts_prosody_control_c(h->text, 62, h->pitch, h->energy, h->dur, pb, pe, B, fit_scales, fit_curves, st));
    else TTS_TRY(tts_prosody_control_v(h->text, 62, h->pitch, h->energy, h->dur, pb, pe, B, fit_scales, st));
    TTS_TRY(tts_prosody_fit_apply(h->dur, fit_extra, R, st));
  } else if (q.curves) {
    TTS_TRY(tts_prosody_control_c(h->text, 62, h->pitch, h->energy, h->dur, pb, pe, B, sdev, cdev, st));
  } else {
    TTS_TRY(tts_prosody_control_v(h->text, 62, h->pitch, h->energy, h->dur, pb, pe, B, sdev, st));
  }
  TTS_TRY(tts_prosody_stats(h->pitch, h->energy, h->dur, pb, pe, B, uafter, st));
  TTS_TRY(tts_prosody_stats(h->pitch, h->energy, h->dur, xb, xe, n_spans, xafter, st));
  h->pstats_host.assign(2 * NU, 0.f);
  TTS_TRY(hip_ok(hipMemcpyAsync(h->pstats_host.data(), ubefore, 2 * NU * sizeof(float), hipMemcpyDeviceToHost, st), "prosody statistics to host"));
  if (q.curves) h->sstats_host.assign(2 * NX, 0.f);
  if (n_spans > 0)
    TTS_TRY(hip_ok(hipMemcpyAsync(h->sstats_host.data(), xbefore, 2 * NX * sizeof(float), hipMemcpyDeviceToHost, st), "span statistics to host"));
  if (fit) {
    const size_t NR = (size_t)n_seg * TTS_FIT_COLUMNS, NS = (size_t)B * TTS_PROSODY_SCALES;
    h->fit_host.assign(NR + NS, 0.f);
    h->fit_extra_host.assign(R, 0);
    TTS_TRY(hip_ok(hipMemcpyAsync(h->fit_host.data(), fit_report, NR * sizeof(float), hipMemcpyDeviceToHost, st), "fit report to host"));
    TTS_TRY(hip_ok(hipMemcpyAsync(h->fit_host.data() + NR, fit_scales, NS * sizeof(float), hipMemcpyDeviceToHost, st), "fitted scales to host"));
    TTS_TRY(hip_ok(hipMemcpyAsync(h->fit_extra_host.data(), fit_extra, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, st), "extra frames to host"));
  }
  const int rc = regulate(h, h->dur, false, frames_out, st);  // (synchronises st once: durations and statistics are on the host)
  if (rc != TTS_OK) h->pstats_host.clear();
  if (fit) {
    h->n_fit = rc == TTS_OK ? n_seg : -1;
    if (rc != TTS_OK) {
      h->fit_host.clear();
      h->fit_extra_host.clear();
    }
  }
  if (q.curves) {
    h->n_spans = rc == TTS_OK ? n_spans : -1;
    if (rc != TTS_OK) h->sstats_host.clear();
  }
  return rc;
}

// ---- stage A.2 + A.3 with teacher forcing (the scorer): raw predictions, gold prosody, gold durations -----------------------
// ToucanTTS._forward, training branch (ToucanTTS.py:321-330): every predictor runs and its raw output is the caller's; the GOLD
// pitch / energy are embedded and the GOLD durations expand the text.  No tts_prosody_control: no overrides, no scales.
int pipeline_teacher_forced(Handle* h, const float* gold_pitch, const float* gold_energy, const int* gold_dur, float* pred_log_dur,
                            float* pred_pitch, float* pred_energy, int* frames_out, hipStream_t st) {
  TTS_CHECK_ARG(h && h->enc, "tts_teacher_forced: run tts_encoder first");
  TTS_CHECK_RESOLVED(h, "tts_teacher_forced");
  TTS_CHECK_ARG(gold_pitch && gold_energy && gold_dur && pred_log_dur && pred_pitch && pred_energy, "tts_teacher_forced: null pointer");
  h->split_mode = 2;
  h->tab_which = 0;
  const Acoustic& m = h->acoustic;
  const int R = h->lp.total;
  if (h->cfg.multispeaker) TTS_TRY(cln_prepare(h, st));
  TTS_TRY(predictor(h, m.pitch, pred_pitch, st));
  TTS_TRY(predictor(h, m.energy, pred_energy, st));
  TTS_TRY(predictor(h, m.duration, pred_log_dur, st));
  TTS_TRY(hip_ok(hipMemcpyAsync(h->pitch, gold_pitch, (size_t)R * 4, hipMemcpyDeviceToDevice, st), "gold pitch"));
  TTS_TRY(hip_ok(hipMemcpyAsync(h->energy, gold_energy, (size_t)R * 4, hipMemcpyDeviceToDevice, st), "gold energy"));
  TTS_TRY(hip_ok(hipMemcpyAsync(h->dur, gold_dur, (size_t)R * 4, hipMemcpyDeviceToDevice, st), "gold durations"));
  return regulate(h, gold_dur, true, frames_out, st);
}

// ---- stage B.1: decoder + feat_out --------------------------------------------------------------------------------------
int pipeline_decoder(Handle* h, hipStream_t st) {
  TTS_CHECK_ARG(h && h->dec, "tts_decoder: run tts_control_and_regulate first");
  TTS_CHECK_RESOLVED(h, "tts_decoder");
  h->split_mode = 1;
  h->tab_which = 0;
  TTS_TRY(conformer(h, 1, h->dec, h->lf, h->frame, st));
  TTS_ALLOC(mel0, h->frame, float, (size_t)h->lf.total * 80);
  h->mel0 = mel0;
  h->mel = nullptr;
  return conv(h, h->acoustic.feat_out, T2(h->dec, ATT), T2(mel0, 80), h->lf, st);
}

// ---- stage B.2: PostNet + residual -------------------------------------------------------------------------------------
int pipeline_postnet(Handle* h, hipStream_t st) {
  TTS_CHECK_ARG(h && h->mel0, "tts_postnet: run tts_decoder first");
  TTS_CHECK_RESOLVED(h, "tts_postnet");
  h->split_mode = 1;
  h->tab_which = 0;
  const Layout& l = h->lf;
  const int RF = l.total;
  Arena& a = h->frame;
  TTS_ALLOC(x, a, float, (size_t)RF * 256);
  TTS_ALLOC(y, a, float, (size_t)RF * 256);
  TTS_ALLOC(y80, a, float, (size_t)RF * 80);
  const long long wsn = std::max<long long>(1, tts_groupnorm_workspace_floats(l.n(), l.max_len, 32));
  TTS_ALLOC(gws, a, float, wsn);
  const int *sb, *se;
  TTS_TRY(bounds_of(h, l, st, &sb, &se));
  const float* src = h->mel0;
  int ld = 80;
  for (int i = 0; i < 5; ++i) {
    const auto& p = h->acoustic.postnet[i];
    if (i < 4) {
      TTS_TRY(conv(h, p.conv, T2(const_cast<float*>(src), ld), T2(x, 256), l, st));
      TTS_TRY(tts_groupnorm(x, 256, y, 256, p.g, p.b, 256, 32, 1e-5f, 1, nullptr, 0, sb, se, l.n(), l.max_len, gws, st));
      src = y;
      ld = 256;
    } else {
      TTS_TRY(conv(h, p.conv, T2(const_cast<float*>(src), ld), T2(y80, 80), l, st));
      TTS_TRY(tts_groupnorm(y80, 80, h->cat, 80 + ATT, p.g, p.b, 80, 20, 1e-5f, 0, h->mel0, 80, sb, se, l.n(), l.max_len, gws, st));
    }
  }
  h->mel = h->cat;  // refined mel, row stride 80 + 192
  h->have_flow = false;
  return TTS_OK;
}

// ---- stage B.3: PostFlow (Glow, reverse pass) ---------------------------------------------------------------------------
// z_noise: [total_frames / 2, 160] = the 0.8 N(0,1) sample in the squeezed layout of the frame layout (rows of utterance u at
// frame_begin[u] / 2; Glow.py:363 draws it inside the model, here it is an explicit input)
int pipeline_postflow(Handle* h, const float* z_noise, hipStream_t st) {
  TTS_CHECK_ARG(h && h->mel == h->cat && h->cat, "tts_postflow: run tts_postnet first");
  TTS_CHECK_ARG(z_noise, "tts_postflow: z_noise is required");
  TTS_CHECK_RESOLVED(h, "tts_postflow");
  h->split_mode = 1;
  h->tab_which = 0;
  const Layout ls = h->lf.halved();
  const int RF = h->lf.total, RS = RF / 2;
  Arena& a = h->frame;
  const int b16 = bits16(h);
  const Acoustic& m = h->acoustic;
  TTS_ALLOC(g, a, float, (size_t)RF * ATT);
  TTS_TRY(conv(h, m.g_proj, T2(h->cat, 80 + ATT), T2(g, ATT), h->lf, st));
  // 16-bit configurations: one launch per coupling block (wavenet_block: start conv, the four layers, end conv with the coupling,
  // inverse 1x1 conv and ActNorm); the hidden state and the skip sum never leave the chip.  A block reads x from one buffer and
  // writes the other (its workgroups read each other's rows of x0): block 17 reads z_noise itself, and the 18 writes alternate
  // between x and x2, so the mel ends in x2 whatever the batch.  The other configurations keep the per-layer launches and x in place.
  const bool fused = !postflow_cond_buffer(h);
  TTS_ALLOC(x, a, float, (size_t)RS * 160);
  float *hs = nullptr, *x2 = nullptr;
  if (fused) {
    x2 = arena_alloc<float>(a, (size_t)RS * 160);
  } else {
    TTS_TRY(hip_ok(hipMemcpyAsync(x, z_noise, (size_t)RS * 160 * 4, hipMemcpyDeviceToDevice, st), "flow noise"));
    hs = arena_alloc<float>(a, (size_t)RS * 2 * ATT);  // [hidden state | skip sum]
  }
  if (!hs && !x2) {
    set_error("tts_postflow: workspace exhausted");
    return TTS_E_ARG;
  }
  TileTab tblk;
  const int* pad_rows = nullptr;  // the squeezed rows outside every tile: the one behind an utterance with an odd frame count
  int n_pad = 0;
  if (fused) {
    TTS_TRY(tiles_of(h, ls, wavenet_block_tile_rows(), st, &tblk));
    void* dev;
    TTS_TRY(table_of(h, layout_key(h->lf, -2), st, [&] {
      std::vector<int> host;
      for (int u = 0; u < h->lf.n(); ++u)
        if (h->lf.lengths[u] & 1) host.push_back(ls.begins[u] + ls.lengths[u]);
      return host;
    }, &dev, &n_pad));
    pad_rows = static_cast<const int*>(dev);
  }
  // the fused layers compute their conditioning columns themselves: no acts, no cond buffer
  char* acts = nullptr;
  float* cond = nullptr;
  if (!fused) {
    acts = arena_alloc<char>(a, (size_t)RS * ATT * (b16 / 8));
    cond = arena_alloc<float>(a, (size_t)RS * 8 * ATT);
    if (!acts || !cond) {
      set_error("tts_postflow: workspace exhausted");
      return TTS_E_ARG;
    }
  }
  float* skip = hs ? hs + ATT : nullptr;
  double live_rows = 0;  // (stage profiler)
  for (int n : ls.lengths) live_rows += n;
  for (int b = 17; b >= 0; --b) {
    const auto& f = m.flow[b];
    const ConvW& cnd = f.cond;
    if (!fused) {
      TTS_TRY(conv(h, f.start, T2(x, 160), T2(hs, 2 * ATT), ls, st));          // h = start(x0); the zero half clears the skip sum
      TTS_TRY(conv(h, cnd, T2(g, 2 * ATT), T2(cond, 8 * ATT), ls, st));        // squeeze of g = re-view [RS, 384]
    }
    if (fused) {
      TTS_CHECK_ARG(f.start.w16 && f.start.mode == TTS_MODE_LINEAR && f.start.compute16 == cnd.compute16 && f.start.cin == 80 && f.start.taps == 1 && f.start.wn >= ATT,
                    "tts_postflow: flow.%d.start is not a 16-bit 1-tap 80 -> 192 conv", b);
      TTS_CHECK_ARG(cnd.w16 && cnd.mode == TTS_MODE_LINEAR && cnd.cin == 2 * ATT && cnd.cin_pad == 2 * ATT && cnd.cout == 8 * ATT && cnd.taps == 1 && cnd.wn >= 8 * ATT,
                    "tts_postflow: flow.%d.cond is not a 16-bit 1-tap 384 -> 1536 conv", b);
      WavenetBlock w;
      memset(&w, 0, sizeof(w));
      TTS_CHECK_ARG(f.end.w && f.end.mode == TTS_MODE_COUPLING && f.end.cin == ATT && f.end.cin_pad == ATT && f.end.cout == 80 && f.end.taps == 1,
                    "tts_postflow: flow.%d.end is not an fp32 1-tap 192 -> 2 x 80 coupling conv", b);
      // block 17 reads the noise where the caller put it; the others what the block before them wrote
      const float* xin = b == 17 ? z_noise : ((b & 1) ? x2 : x);
      float* xout = (b & 1) ? x : x2;
      w.x = xin; w.ld_x = 160; w.x_out = xout; w.ld_out = 160;
      w.we = f.end.w; w.we_n = f.end.wn; w.we_half = f.end.half_pad; w.be = f.end.bias; w.alpha = ConvOpt().alpha;
      w.winv = f.winv; w.an_bias = f.an_bias; w.an_logs = f.an_logs;
      w.pad_rows = pad_rows; w.n_pad = n_pad;
      w.w0 = f.start.w16; w.w0_n = f.start.wn; w.b0 = f.start.bias;
      w.g = g; w.ld_g = 2 * ATT; w.wc = cnd.w16; w.wc_n = cnd.wn; w.bc = cnd.bias;
      w.tiles = tblk.dev; w.n_tiles = tblk.n; w.tile_rows = wavenet_block_tile_rows();
      w.compute = cnd.compute16;
      for (int i = 0; i < 4; ++i) {
        const ConvW &inl = m.flowgrp[b / 4].inl[i], &rs = m.flowgrp[b / 4].res_skip[i];
        TTS_CHECK_ARG(inl.w16 && rs.w16 && inl.compute16 == cnd.compute16 && rs.cout == (i < 3 ? 2 * ATT : ATT), "tts_postflow: flow.%d layer %d is not a 16-bit WaveNet layer", b, i);
        w.w1[i] = inl.w16; w.b1[i] = inl.bias; w.w2[i] = rs.w16; w.b2[i] = rs.bias;
      }
      // start, four layers' in-layer, conditioning and res/skip products, end and the 4 x 4 mix of 40 groups (the halo's repeated
      // rows are not counted); x in, x out, g, the 16-bit weights and end's fp32 ones
      TTS_TRY(prof_launch(h, "wavenet_block",
                          2.0 * live_rows * (80.0 * ATT + 4.0 * (ATT * 5 * 2 * ATT + 2 * ATT * 2 * ATT) + 3.0 * ATT * 2 * ATT + (double)ATT * ATT + ATT * 160.0 + 160.0 * 4),
                          live_rows * 4.0 * (160 + 160 + 2 * ATT) + 2.0 * (80.0 * ATT + 4.0 * (5 * ATT * 2 * ATT + 2 * ATT * 2 * ATT) + 3.0 * ATT * 2 * ATT + (double)ATT * ATT) + 4.0 * ATT * 160,
                          live_rows * 160, st, [&] { return wavenet_block(w, st); }));
      continue;
    }
    for (int i = 0; i < 4 && !fused; ++i) {
      const ConvW &inl = m.flowgrp[b / 4].inl[i], &rs = m.flowgrp[b / 4].res_skip[i];
      ConvOpt oi;
      oi.preadd = cond + (size_t)i * 2 * ATT;
      oi.ld_preadd = 8 * ATT;
      TTS_TRY(conv(h, inl, T2(hs, 2 * ATT), T2(acts, ATT, b16), ls, st, oi));
      ConvOpt orr;
      orr.accumulate = true;
      TTS_TRY(conv(h, rs, T2(acts, ATT, b16), i < 3 ? T2(hs, 2 * ATT) : T2(skip, 2 * ATT), ls, st, orr));
    }
    ConvOpt oe;
    oe.aux = x + 80;
    oe.ld_aux = 160;
    oe.fp32_only = true;
    TTS_TRY(conv(h, f.end, T2(skip, 2 * ATT), T2(x + 80, 160), ls, st, oe));
    TTS_TRY(tts_glow_invconv_actnorm(x, 160, RS, 160, f.winv, f.an_bias, f.an_logs, st));
  }
  h->mel = fused ? x2 : x;  // (block 0 wrote x2) unsqueeze = re-view [2 RS, 80]
  h->have_flow = true;
  return TTS_OK;
}

// ---- the scorer's glow loss: PostFlow, forward pass (Glow.forward(infer=False), Glow.py:350-360) -----------------------------
// gold [RF, 80] (row stride ld_gold) -> z by the 18 blocks in their own order: ActNorm, InvConvNear, coupling.  The conditioning and
// the WaveNet of a coupling block are one function in both directions, so they are the conv launches of pipeline_postflow's fp32
// branch; `end` runs as a plain conv into [m | logs], and tts_glow_forward_rows does the rest of a step: the coupling of block b
// with ActNorm and InvConv of block b + 1 (19 launches).  tts_glow_nll_reduce turns z and the row log-determinants into the loss.
// The frame arena is used from where tts_postnet left it and handed back as it was: tts_postflow can follow.  The mel is not touched.
struct ArenaRewind {
  Arena& a;
  size_t off;
  explicit ArenaRewind(Arena& a_) : a(a_), off(a_.off) {}
  ~ArenaRewind() { a.off = off; }
};

int pipeline_postflow_nll(Handle* h, const float* gold, int ld_gold, float* loss, float* row_parts, float* z_out, hipStream_t st) {
  TTS_CHECK_ARG(h, "tts_postflow_nll: null handle");
  TTS_CHECK_ARG(!is16(h), "tts_postflow_nll: fp32 handles only (this one was created with precision %d)", h->cfg.precision);
  TTS_CHECK_ARG(find(h, "flow.logdet") && find(h, "flow.0.wfwd") && find(h, "flow.0.end_ml.w"),
                "tts_postflow_nll: the forward weights flow.<b>.wfwd, flow.<b>.end_ml and flow.logdet were not loaded (tts_load_weights; "
                "NativePipeline(..., scoring=True) uploads them)");
  TTS_CHECK_ARG(h->mel == h->cat && h->cat, "tts_postflow_nll: run tts_postnet first");
  TTS_CHECK_ARG(gold && ld_gold >= 80 && loss, "tts_postflow_nll: null gold_mel / loss_out, or row stride %d < 80", ld_gold);
  TTS_CHECK_RESOLVED(h, "tts_postflow_nll");
  const Acoustic& m = h->acoustic;
  TTS_CHECK_ARG(m.scoring, "tts_postflow_nll: the forward weights were not resolved: run tts_encoder again");
  h->split_mode = 1;
  h->tab_which = 0;
  const Layout ls = h->lf.halved();
  const int RF = h->lf.total, RS = RF / 2, B = h->lf.n();
  long long live_rows = 0;
  for (int n : ls.lengths) live_rows += n;
  // its own scratch: [m | logs] of a block's `end` conv and one fp64 log-determinant per row
  const size_t ml_bytes = ((size_t)RS * 160 * 4 + 255) & ~(size_t)255, ld_bytes = ((size_t)RS * 8 + 255) & ~(size_t)255;
  TTS_TRY(arena_reserve(h->nll, ml_bytes + ld_bytes, st));
  TTS_ALLOC(ml, h->nll, float, (size_t)RS * 160);
  TTS_ALLOC(row_logdet, h->nll, double, RS);
  TTS_TRY(hip_ok(hipMemsetAsync(h->nll.base, 0, ml_bytes + ld_bytes, st), "tts_postflow_nll: clear scratch"));  // (rows between utterances: m = logs = 0)
  void* tab;
  TTS_TRY(table_of(h, layout_key(h->lf, -2), st, [&] {  // (row_begin[B] | n_rows[B] | n_frames[B])
    std::vector<int> host(3 * (size_t)B);
    for (int u = 0; u < B; ++u) {
      host[u] = ls.begins[u];
      host[B + u] = ls.lengths[u];
      host[2 * B + u] = h->lf.lengths[u];
    }
    return host;
  }, &tab, nullptr));
  const int* utt = static_cast<const int*>(tab);
  Arena& a = h->frame;
  ArenaRewind rewind(a);
  TTS_ALLOC(x, a, float, (size_t)RS * 160);
  TTS_TRY(hip_ok(hipMemcpy2DAsync(x, 80 * 4, gold, (size_t)ld_gold * 4, 80 * 4, RF, hipMemcpyDeviceToDevice, st), "tts_postflow_nll: gold mel"));
  if (live_rows > 0) {  // (a batch of one-frame utterances launches nothing but the reduction)
    TTS_ALLOC(g, a, float, (size_t)RF * ATT);
    TTS_TRY(conv(h, m.g_proj, T2(h->cat, 80 + ATT), T2(g, ATT), h->lf, st));
    TTS_ALLOC(hs, a, float, (size_t)RS * 2 * ATT);  // [hidden state | skip sum]
    TTS_ALLOC(acts, a, float, (size_t)RS * ATT);
    TTS_ALLOC(cond, a, float, (size_t)RS * 8 * ATT);
    float* skip = hs + ATT;
    TTS_TRY(tts_glow_forward_rows(x, 160, RS, nullptr, 0, nullptr, m.flow_fwd[0].wfwd, m.flow[0].an_bias, m.flow[0].an_logs, st));
    for (int b = 0; b < 18; ++b) {
      const auto& f = m.flow[b];
      TTS_TRY(conv(h, f.start, T2(x, 160), T2(hs, 2 * ATT), ls, st));      // h = start(x0); the zero half clears the skip sum
      TTS_TRY(conv(h, f.cond, T2(g, 2 * ATT), T2(cond, 8 * ATT), ls, st));  // squeeze of g = re-view [RS, 384]
      for (int i = 0; i < 4; ++i) {
        const ConvW &inl = m.flowgrp[b / 4].inl[i], &rs = m.flowgrp[b / 4].res_skip[i];
        ConvOpt oi;
        oi.preadd = cond + (size_t)i * 2 * ATT;
        oi.ld_preadd = 8 * ATT;
        TTS_TRY(conv(h, inl, T2(hs, 2 * ATT), T2(acts, ATT), ls, st, oi));
        ConvOpt orr;
        orr.accumulate = true;
        TTS_TRY(conv(h, rs, T2(acts, ATT), i < 3 ? T2(hs, 2 * ATT) : T2(skip, 2 * ATT), ls, st, orr));
      }
      ConvOpt oe;
      oe.fp32_only = true;
      TTS_TRY(conv(h, m.flow_fwd[b].end_ml, T2(skip, 2 * ATT), T2(ml, 160), ls, st, oe));
      const bool last = b == 17;
      TTS_TRY(tts_glow_forward_rows(x, 160, RS, ml, 160, row_logdet, last ? nullptr : m.flow_fwd[b + 1].wfwd, last ? nullptr : m.flow[b + 1].an_bias,
                                    last ? nullptr : m.flow[b + 1].an_logs, st));
    }
  }
  TTS_TRY(tts_glow_nll_reduce(x, 160, row_logdet, utt, utt + B, utt + 2 * B, B, m.flow_logdet, loss, row_parts, st));
  if (z_out) TTS_TRY(hip_ok(hipMemcpyAsync(z_out, x, (size_t)RS * 160 * 4, hipMemcpyDeviceToDevice, st), "tts_postflow_nll: z_out"));
  return TTS_OK;
}

// where the batch's mel lives: packed [rows, 80] with row stride *ld; utterance u at frame_begin[u] (2-aligned), frames[u]
// frames (one fewer than predicted for an odd count once the flow has run)
int pipeline_mel(Handle* h, const float** mel, int* ld, int* frame_begins, int* frame_counts) {
  TTS_CHECK_ARG(h && h->mel, "tts_mel: no mel yet");
  *mel = h->mel;
  *ld = h->have_flow ? 80 : 80 + ATT;
  for (int u = 0; u < h->B; ++u) {
    if (frame_begins) frame_begins[u] = h->lf.begins[u];
    if (frame_counts) frame_counts[u] = h->have_flow ? h->lf.lengths[u] / 2 * 2 : h->lf.lengths[u];
  }
  return TTS_OK;
}

// ---- vocoders ------------------------------------------------------------------------------------------------------------
int pipeline_vocoder(Handle* h, int kind, const float* mel, int ld_mel, const int* frame_begins, const int* frame_counts, int B, float* wav,
                     hipStream_t st) {
  TTS_CHECK_ARG(h && mel && frame_begins && frame_counts && wav && B > 0, "tts_vocoder: bad arguments");
  TTS_CHECK_ARG(kind == h->cfg.vocoder, "tts_vocoder: the handle was created for vocoder %d, not %d", h->cfg.vocoder, kind);
  TTS_TRY(resolve_vocoder(h));  // (before anything is reserved or enqueued, like the acoustic model in tts_encoder)
  const Vocoder& m = h->vocoder;
  h->split_mode = 0;
  TTS_TRY(tables_begin(h, 1, st));
  const bool big = kind == 2;
  Layout l;
  for (int u = 0; u < B; ++u) {
    l.begins.push_back(frame_begins[u]);
    l.lengths.push_back(frame_counts[u]);
    l.total = std::max(l.total, frame_begins[u] + frame_counts[u]);
    l.max_len = std::max(l.max_len, frame_counts[u]);
  }
  const int b16 = bits16(h);
  const bool fused_mode = b16 == 16;  // 16-bit configurations run the fused residual step for C <= 128 and keep 16-bit residual streams
  const size_t e = b16 / 8;
  size_t R = l.total;
  // stage buffers: x (input of the stage) lives in the other arena
  // both arenas at their size for the whole pass (the larger of the stages each one hosts: a stage would otherwise regrow the arena
  // its predecessor's input still lives in)
  const size_t R0 = R;
  TTS_TRY(arena_reserve(h->voc[1], vocoder_arena_bytes(R0, 1, fused_mode, big), st));
  TTS_TRY(arena_reserve(h->voc[0], vocoder_arena_bytes(R0, 0, fused_mode, big), st));
  TTS_ALLOC(x0, h->voc[1], float, R * 512);
  TTS_TRY(conv(h, m.pre, T2(const_cast<float*>(mel), ld_mel), T2(x0, 512), l, st));
  T2 x(x0, 512);
  static const int UP[4] = {8, 6, 4, 2};
  int ch = 512;
  for (int i = 0; i < 4; ++i) {
    ch /= 2;
    const int u = UP[i];
    const bool fused = fused_mode && ch <= 128;
    const int sb = fused_mode ? 16 : 32;  // element size of the stage's tensors
    const size_t se = sb / 8;
    Arena& a = h->voc[i & 1];
    const size_t RU = R * u;
    a.reset();  // (sized above; the stage two steps back is dead)
    TTS_ALLOC(y, a, char, RU * ch * se);
    ConvOpt ou;
    if (!big) { ou.pre = TTS_PRE_LRELU; ou.pre_slope = 0.1f; }
    TTS_TRY(conv(h, m.ups[i], x, T2(y, u * ch, sb), l, st, ou));  // transposed conv as a 3-tap polyphase conv; [R, u ch] re-viewed as [R u, ch]
    R = RU;
    l = l.scaled(u);
    TTS_ALLOC(stage_out, a, char, R * ch * se);
    TTS_ALLOC(buf0, a, char, R * ch * se);
    TTS_ALLOC(buf1, a, char, R * ch * se);
    char *t1 = nullptr, *t2 = nullptr, *sa = nullptr;
    if (!fused) {
      t1 = arena_alloc<char>(a, R * ch * se);
      if (big) {
        t2 = arena_alloc<char>(a, R * ch * se);
        sa = arena_alloc<char>(a, R * ch * se);
      }
      if (!t1 || (big && (!t2 || !sa))) {
        set_error("tts_vocoder: workspace exhausted");
        return TTS_E_ARG;
      }
    }
    TileTab trb, t256;
    if (fused) TTS_TRY(tiles_of(h, l, tts_resblock_tile_rows(ch), st, &trb));
    if (big && !fused) TTS_TRY(tiles_of(h, l, 256, st, &t256));
    const int f16flag = (sb == 16 && h->cfg.precision == TTS_COMPUTE_F16) ? TTS_IO_F16 : 0;
    char pname[32];  // (stage profiler)
    snprintf(pname, sizeof(pname), "resblock_step<%d>", ch);
    double live_rows = 0;
    for (int n : l.lengths) live_rows += n;
    for (int j = 0; j < 3; ++j) {
      char* cur = y;
      char* bufs[2] = {buf0, buf1};
      for (int dd = 0; dd < 3; ++dd) {
        const auto& k = m.blk[i][j][dd];
        const ConvW &c1 = k.c1, &c2 = k.c2;
        const bool last = dd == 2;
        char* dst = last ? stage_out : bufs[dd % 2];
        if (fused) {  // one launch per dilation step: act, conv(dil), act, conv(1), + x (and the stage mean on the last step)
          TtsResblockDesc r;
          memset(&r, 0, sizeof(r));
          r.x = reinterpret_cast<const float*>(cur); r.ldx = ch; r.y = reinterpret_cast<float*>(dst); r.ldy = ch;
          r.c = ch; r.taps = c1.taps; r.dil = c1.dil;
          r.w1 = c1.w16; r.b1 = c1.bias; r.w2 = c2.w16; r.b2 = c2.bias;
          r.act = big ? TTS_PRE_SNAKE : TTS_PRE_LRELU; r.slope = 0.1f;
          r.alpha1 = k.a1; r.beta1 = k.b1; r.alpha2 = k.a2; r.beta2 = k.b2; r.filt = m.filt; r.fir_tab = m.fir_tab;
          r.alpha = last ? 1.0f / 3.0f : 1.0f; r.res_scale = r.alpha; r.accumulate = (last && j > 0) ? 1 : 0;
          r.io_bf16 = 1; r.tiles = trb.dev; r.n_tiles = trb.n; r.tile_rows = tts_resblock_tile_rows(ch); r.compute = c1.compute16;
          TTS_TRY(prof_launch(h, pname, 2.0 * live_rows * ch * ch * c1.taps * 2, 2.0 * live_rows * ch * se + 2.0 * c1.taps * ch * ch * 2, live_rows * ch, st,
                              [&] { return tts_resblock_step(&r, st); }));
          cur = dst;
          continue;
        }
        T2 src2;
        ConvOpt o2;
        if (big) {  // AMP.py:51-60: a1 -> c1 -> a2 -> c2 -> + x with stand-alone anti-aliased snakes
          const int fl = (sb == 16 ? (TTS_IO_X_BF16 | TTS_IO_Y_BF16) : 0) | f16flag;
          TTS_TRY(tts_snake_aa(reinterpret_cast<const float*>(cur), ch, reinterpret_cast<float*>(sa), ch, k.a1, k.b1, m.filt, ch, t256.dev, t256.n, 256, fl, st));
          TTS_TRY(conv(h, c1, T2(sa, ch, sb), T2(t1, ch, sb), l, st));
          TTS_TRY(tts_snake_aa(reinterpret_cast<const float*>(t1), ch, reinterpret_cast<float*>(t2), ch, k.a2, k.b2, m.filt, ch, t256.dev, t256.n, 256, fl, st));
          src2 = T2(t2, ch, sb);
        } else {  // ResidualBlock.py:83-98 with LeakyReLU(0.1)
          ConvOpt o1;
          o1.pre = TTS_PRE_LRELU; o1.pre_slope = 0.1f;
          TTS_TRY(conv(h, c1, T2(cur, ch, sb), T2(t1, ch, sb), l, st, o1));
          src2 = T2(t1, ch, sb);
          o2.pre = TTS_PRE_LRELU; o2.pre_slope = 0.1f;
        }
        o2.res = T2(cur, ch, sb);
        if (last) {  // stage output = mean of the three blocks (InferenceBigVGAN.py:82-88)
          o2.alpha = 1.0f / 3.0f; o2.res_scale = 1.0f / 3.0f; o2.accumulate = j > 0;
        }
        TTS_TRY(conv(h, c2, src2, T2(dst, ch, sb), l, st, o2));
        cur = dst;
      }
    }
    x = T2(stage_out, ch, sb);
  }
  const int xflag = (x.bits == 16 ? TTS_IO_X_BF16 : 0) | ((x.bits == 16 && h->cfg.precision == TTS_COMPUTE_F16) ? TTS_IO_F16 : 0);
  if (big) {
    TileTab tp;
    const int tr = tts_conv_post_snake_tile_rows();
    TTS_TRY(tiles_of(h, l, tr, st, &tp));
    return tts_conv_post_snake(static_cast<const float*>(x.p), ch, ch, m.post_w, h->cfg.post_bias, m.post_a, m.post_b, m.filt, wav, tp.dev, tp.n, tr, xflag, st);
  }
  TileTab tp;
  TTS_TRY(tiles_of(h, l, 256, st, &tp));
  return tts_conv_post(static_cast<const float*>(x.p), ch, ch, m.post_w, h->cfg.post_bias, TTS_PRE_LRELU, 0.01f, wav, tp.dev, tp.n, 256, xflag, st);  // InferenceAvocodo.py:53
}

// the end of every stage entry, whatever its outcome (the extern "C" wrappers): the table generation of `group` that the running batch
// uses was last used on st.  rc: the entry's own status, which comes first
int stage_done(Handle* h, int group, hipStream_t st, int rc) {
  if (!h) return rc;
  TableStore& s = h->tabs[group][h->tab_gen[group]];
  hipError_t e = hipSuccess;
  if (!s.last_use && (e = hipEventCreateWithFlags(&s.last_use, hipEventDisableTiming)) != hipSuccess) s.last_use = nullptr;
  if (e == hipSuccess) e = hipEventRecord(s.last_use, st);
  return rc != TTS_OK ? rc : hip_ok(e, "tile tables: last use");
}

}  // namespace tts

// ======================================================================================================================
extern "C" {

#define H(h) reinterpret_cast<tts::Handle*>(h)
#define ST(s) reinterpret_cast<hipStream_t>(s)

int tts_create(const TtsConfig* cfg, TtsHandle** out) { return tts::pipeline_create(cfg, reinterpret_cast<tts::Handle**>(out)); }
int tts_destroy(TtsHandle* h) { return tts::pipeline_destroy(H(h)); }
int tts_load_weights(TtsHandle* h, const char* name, const void* host_ptr, const int64_t* shape, int32_t ndim, int32_t dtype) {
  return tts::pipeline_load(H(h), name, host_ptr, shape, ndim, dtype);
}
int64_t tts_workspace_bytes(const TtsHandle* h, int32_t B, int32_t Lmax, int32_t Tmax) {
  return tts::pipeline_workspace_bytes(reinterpret_cast<const tts::Handle*>(h), B, Lmax, Tmax);
}
int64_t tts_workspace_claimed(const TtsHandle* h) { return tts::pipeline_workspace_claimed(reinterpret_cast<const tts::Handle*>(h)); }
int tts_table_stats(const TtsHandle* h, int64_t* tables_built, int64_t* table_chunks) {
  if (!h || !tables_built || !table_chunks) return TTS_E_ARG;
  const tts::Handle* hh = reinterpret_cast<const tts::Handle*>(h);
  *tables_built = hh->n_tables_built;
  *table_chunks = 0;
  for (const auto& group : hh->tabs)
    for (const tts::TableStore& s : group) *table_chunks += (int64_t)s.chunks.size();
  return TTS_OK;
}
int tts_encoder(TtsHandle* h, const float* text, const float* utt_emb, const int32_t* lang_ids, const int32_t* phone_lengths, int32_t B,
                tts_stream_t stream) {
  return tts::stage_done(H(h), 0, ST(stream), tts::pipeline_encoder(H(h), text, utt_emb, lang_ids, phone_lengths, B, ST(stream)));
}
int tts_variance_predictors(TtsHandle* h, const float* gold_pitch, const float* gold_energy, const int32_t* gold_durations, tts_stream_t stream) {
  return tts::stage_done(H(h), 0, ST(stream), tts::pipeline_predictors(H(h), gold_pitch, gold_energy, gold_durations, ST(stream)));
}
int tts_control_and_regulate(TtsHandle* h, float duration_scale, float pitch_scale, float energy_scale, float pause_scale,
                             int32_t* frame_counts, tts_stream_t stream) {
  tts::ControlRequest q{"tts_control_and_regulate", tts::ControlRequest::BATCH, {duration_scale, pitch_scale, energy_scale, pause_scale}};
  return tts::stage_done(H(h), 0, ST(stream), tts::control_regulate(H(h), q, frame_counts, ST(stream)));
}
int tts_control_and_regulate_v(TtsHandle* h, const float* scales, int32_t* frame_counts, tts_stream_t stream) {
  tts::ControlRequest q{"tts_control_and_regulate_v", tts::ControlRequest::UTTERANCE};
  q.scales = scales;
  return tts::stage_done(H(h), 0, ST(stream), tts::control_regulate(H(h), q, frame_counts, ST(stream)));
}
int tts_copy_prosody_stats(TtsHandle* h, float* before, float* after, tts_stream_t stream) {
  (void)stream;  // (the blocks came back with the durations: a host copy)
  tts::Handle* hh = H(h);
  if (!hh || hh->pstats_host.empty()) {
    tts::set_error("tts_copy_prosody_stats: the batch in flight did not go through tts_control_and_regulate_v");
    return TTS_E_ARG;
  }
  const size_t n = (size_t)hh->B * TTS_PROSODY_STATS;
  if (before) memcpy(before, hh->pstats_host.data(), n * sizeof(float));
  if (after) memcpy(after, hh->pstats_host.data() + n, n * sizeof(float));
  return TTS_OK;
}
int tts_control_and_regulate_c(TtsHandle* h, const float* scales, const float* curves, const int32_t* spans, int32_t n_spans,
                               int32_t* frame_counts, tts_stream_t stream) {
  tts::ControlRequest q{"tts_control_and_regulate_c", tts::ControlRequest::PHONEME};
  q.scales = scales;
  q.curves = curves;
  q.spans = spans;
  q.n_spans = n_spans;
  return tts::stage_done(H(h), 0, ST(stream), tts::control_regulate(H(h), q, frame_counts, ST(stream)));
}
int tts_control_and_regulate_t(TtsHandle* h, const float* scales, const float* curves, const int32_t* spans, int32_t n_spans,
                               const float* segments, int32_t n_seg, int32_t* frame_counts, tts_stream_t stream) {
  tts::ControlRequest q{"tts_control_and_regulate_t", tts::ControlRequest::FIT};
  q.scales = scales;
  q.curves = curves;
  q.spans = spans;
  q.n_spans = n_spans;
  q.segments = segments;
  q.n_seg = n_seg;
  return tts::stage_done(H(h), 0, ST(stream), tts::control_regulate(H(h), q, frame_counts, ST(stream)));
}
int tts_copy_prosody_fit(TtsHandle* h, float* report, float* scales, int32_t* extra, tts_stream_t stream) {
  (void)stream;  // (everything came back with the durations: a host copy)
  tts::Handle* hh = H(h);
  if (!hh || hh->n_fit < 0) {
    tts::set_error("tts_copy_prosody_fit: the batch in flight did not go through tts_control_and_regulate_t");
    return TTS_E_ARG;
  }
  const size_t nr = (size_t)hh->n_fit * TTS_FIT_COLUMNS, ns = (size_t)hh->B * TTS_PROSODY_SCALES;
  if (report) memcpy(report, hh->fit_host.data(), nr * sizeof(float));
  if (scales) memcpy(scales, hh->fit_host.data() + nr, ns * sizeof(float));
  if (extra && !hh->fit_extra_host.empty()) memcpy(extra, hh->fit_extra_host.data(), hh->fit_extra_host.size() * sizeof(int32_t));
  return TTS_OK;
}
int tts_copy_prosody_span_stats(TtsHandle* h, float* before, float* after, tts_stream_t stream) {
  (void)stream;  // (the blocks came back with the durations: a host copy)
  tts::Handle* hh = H(h);
  if (!hh || hh->n_spans < 0) {
    tts::set_error("tts_copy_prosody_span_stats: the batch in flight did not go through tts_control_and_regulate_c");
    return TTS_E_ARG;
  }
  const size_t n = (size_t)hh->n_spans * TTS_PROSODY_STATS;
  if (before && n) memcpy(before, hh->sstats_host.data(), n * sizeof(float));
  if (after && n) memcpy(after, hh->sstats_host.data() + n, n * sizeof(float));
  return TTS_OK;
}
int tts_teacher_forced(TtsHandle* h, const float* gold_pitch, const float* gold_energy, const int32_t* gold_durations, float* pred_log_dur,
                       float* pred_pitch, float* pred_energy, int32_t* frame_counts, tts_stream_t stream) {
  return tts::stage_done(H(h), 0, ST(stream),
                         tts::pipeline_teacher_forced(H(h), gold_pitch, gold_energy, gold_durations, pred_log_dur, pred_pitch, pred_energy,
                                                      frame_counts, ST(stream)));
}
int tts_decoder(TtsHandle* h, tts_stream_t stream) { return tts::stage_done(H(h), 0, ST(stream), tts::pipeline_decoder(H(h), ST(stream))); }
int tts_postnet(TtsHandle* h, tts_stream_t stream) { return tts::stage_done(H(h), 0, ST(stream), tts::pipeline_postnet(H(h), ST(stream))); }
int tts_postflow(TtsHandle* h, const float* z_noise, tts_stream_t stream) {
  return tts::stage_done(H(h), 0, ST(stream), tts::pipeline_postflow(H(h), z_noise, ST(stream)));
}
int tts_postflow_nll(TtsHandle* h, const float* gold_mel, int32_t ld, float* loss_out, float* row_parts_out, float* z_out, tts_stream_t stream) {
  return tts::stage_done(H(h), 0, ST(stream), tts::pipeline_postflow_nll(H(h), gold_mel, ld, loss_out, row_parts_out, z_out, ST(stream)));
}
int tts_mel(TtsHandle* h, const float** mel, int32_t* ld, int32_t* frame_begins, int32_t* frame_counts) {
  return tts::pipeline_mel(H(h), mel, ld, frame_begins, frame_counts);
}
int tts_prosody(TtsHandle* h, const int32_t** durations, const float** pitch, const float** energy) {
  tts::Handle* hh = H(h);
  if (!hh || !hh->dur) {
    tts::set_error("tts_prosody: no batch in flight");
    return TTS_E_ARG;
  }
  if (durations) *durations = hh->dur;
  if (pitch) *pitch = hh->pitch;
  if (energy) *energy = hh->energy;
  return TTS_OK;
}
int tts_profile(TtsHandle* h, int32_t enable, const char* select) {
  tts::Handle* hh = H(h);
  if (!hh) {
    tts::set_error("tts_profile: null handle");
    return TTS_E_ARG;
  }
  for (auto& r : hh->prof) {
    hh->event_pool.push_back(r.e0);
    hh->event_pool.push_back(r.e1);
  }
  hh->prof.clear();
  hh->prof_on = enable != 0;
  hh->prof_detail = enable == 2;  // 2: conv classes carry their shape ("conv1d_bf16<64x64>[192x384 k5 r10240]")
  hh->prof_select = select ? select : "";
  return TTS_OK;
}
int32_t tts_profile_count(TtsHandle* h) { return h ? (int32_t)H(h)->prof.size() : 0; }
int tts_profile_read(TtsHandle* h, int32_t index, char* name, int32_t name_cap, double* ms, double* flops, double* bytes, double* elems) {
  tts::Handle* hh = H(h);
  if (!hh || index < 0 || index >= (int32_t)hh->prof.size()) {
    tts::set_error("tts_profile_read: index %d out of range", index);
    return TTS_E_ARG;
  }
  const tts::ProfRec& r = hh->prof[index];
  float t = 0.f;
  const hipError_t e = hipEventSynchronize(r.e1);
  if (e != hipSuccess || hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) {
    tts::set_error("tts_profile_read: event timing failed");
    return TTS_E_LAUNCH;
  }
  if (name && name_cap > 0) snprintf(name, name_cap, "%s", r.name.c_str());
  if (ms) *ms = t;
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  if (elems) *elems = r.elems;
  return TTS_OK;
}
int tts_copy_prosody(TtsHandle* h, int32_t* durations, float* pitch, float* energy, tts_stream_t stream) {
  tts::Handle* hh = H(h);
  if (!hh || !hh->dur) {
    tts::set_error("tts_copy_prosody: no batch in flight");
    return TTS_E_ARG;
  }
  const size_t n = (size_t)hh->lp.total * 4;
  hipError_t e = hipSuccess;
  if (durations) e = hipMemcpyAsync(durations, hh->dur, n, hipMemcpyDeviceToDevice, ST(stream));
  if (e == hipSuccess && pitch) e = hipMemcpyAsync(pitch, hh->pitch, n, hipMemcpyDeviceToDevice, ST(stream));
  if (e == hipSuccess && energy) e = hipMemcpyAsync(energy, hh->energy, n, hipMemcpyDeviceToDevice, ST(stream));
  if (e != hipSuccess) {
    tts::set_error("tts_copy_prosody: %s", hipGetErrorString(e));
    return TTS_E_LAUNCH;
  }
  return TTS_OK;
}
int tts_copy_mel(TtsHandle* h, float* dst, int32_t ld_dst, tts_stream_t stream) {
  tts::Handle* hh = H(h);
  if (!hh || !hh->mel || !dst) {
    tts::set_error("tts_copy_mel: no mel yet / null destination");
    return TTS_E_ARG;
  }
  const int ld = hh->have_flow ? 80 : 80 + tts::ATT;
  const hipError_t e = hipMemcpy2DAsync(dst, (size_t)ld_dst * 4, hh->mel, (size_t)ld * 4, 80 * 4, hh->lf.total, hipMemcpyDeviceToDevice, ST(stream));
  if (e != hipSuccess) {
    tts::set_error("tts_copy_mel: %s", hipGetErrorString(e));
    return TTS_E_LAUNCH;
  }
  return TTS_OK;
}
int tts_copy_decoder_mel(TtsHandle* h, float* dst, int32_t ld_dst, tts_stream_t stream) {
  tts::Handle* hh = H(h);
  if (!hh || !hh->mel0 || !dst || ld_dst < 80) {
    tts::set_error("tts_copy_decoder_mel: no decoder output yet / null destination / row stride %d < 80", (int)ld_dst);
    return TTS_E_ARG;
  }
  const hipError_t e = hipMemcpy2DAsync(dst, (size_t)ld_dst * 4, hh->mel0, 80 * 4, 80 * 4, hh->lf.total, hipMemcpyDeviceToDevice, ST(stream));
  if (e != hipSuccess) {
    tts::set_error("tts_copy_decoder_mel: %s", hipGetErrorString(e));
    return TTS_E_LAUNCH;
  }
  return TTS_OK;
}
int tts_vocoder_bigvgan(TtsHandle* h, const float* mel, int32_t ld_mel, const int32_t* frame_begins, const int32_t* frame_counts, int32_t B,
                        float* wav, tts_stream_t stream) {
  return tts::stage_done(H(h), 1, ST(stream), tts::pipeline_vocoder(H(h), 2, mel, ld_mel, frame_begins, frame_counts, B, wav, ST(stream)));
}
int tts_vocoder_hifigan(TtsHandle* h, const float* mel, int32_t ld_mel, const int32_t* frame_begins, const int32_t* frame_counts, int32_t B,
                        float* wav, tts_stream_t stream) {
  return tts::stage_done(H(h), 1, ST(stream), tts::pipeline_vocoder(H(h), 1, mel, ld_mel, frame_begins, frame_counts, B, wav, ST(stream)));
}

// The whole pass for one ragged batch.  z_noise == NULL skips the flow (the refined mel is vocoded); wav == NULL skips the vocoder.
// wav_capacity: samples the caller's buffer holds; needs 384 * (last frame_begin + frame_count) - returned through *wav_needed
// when it does not fit (TTS_E_ARG), so that a caller can size the buffer and call tts_vocoder_* on tts_mel()'s result.
int tts_synthesize_batch(TtsHandle* h, const float* text, const float* utt_emb, const int32_t* lang_ids, const int32_t* phone_lengths,
                         int32_t B, const float* gold_pitch, const float* gold_energy, const int32_t* gold_durations, float duration_scale,
                         float pitch_scale, float energy_scale, float pause_scale, const float* z_noise, int32_t* frame_begins,
                         int32_t* frame_counts, float* wav, int64_t wav_capacity, int64_t* wav_needed, tts_stream_t stream) {
  tts::Handle* hh = H(h);
  int rc;
  if ((rc = tts_encoder(h, text, utt_emb, lang_ids, phone_lengths, B, stream)) != TTS_OK) return rc;
  if ((rc = tts_variance_predictors(h, gold_pitch, gold_energy, gold_durations, stream)) != TTS_OK) return rc;
  if ((rc = tts_control_and_regulate(h, duration_scale, pitch_scale, energy_scale, pause_scale, nullptr, stream)) != TTS_OK) return rc;
  if ((rc = tts_decoder(h, stream)) != TTS_OK) return rc;
  if ((rc = tts_postnet(h, stream)) != TTS_OK) return rc;
  if (z_noise && (rc = tts_postflow(h, z_noise, stream)) != TTS_OK) return rc;
  const float* mel;
  int32_t ld;
  std::vector<int32_t> fb(B), fc(B);
  if ((rc = tts_mel(h, &mel, &ld, fb.data(), fc.data())) != TTS_OK) return rc;
  int64_t need = 0;
  for (int u = 0; u < B; ++u) {
    if (frame_begins) frame_begins[u] = fb[u];
    if (frame_counts) frame_counts[u] = fc[u];
    need = std::max<int64_t>(need, 384ll * (fb[u] + fc[u]));
  }
  if (wav_needed) *wav_needed = need;
  if (!wav || hh->cfg.vocoder == 0) return TTS_OK;
  if (wav_capacity < need) {
    tts::set_error("tts_synthesize_batch: the waveform buffer holds %lld samples, %lld are needed", (long long)wav_capacity, (long long)need);
    return TTS_E_ARG;
  }
  return hh->cfg.vocoder == 2 ? tts_vocoder_bigvgan(h, mel, ld, fb.data(), fc.data(), B, wav, stream)
                              : tts_vocoder_hifigan(h, mel, ld, fb.data(), fc.data(), B, wav, stream);
}

}  // extern "C"
