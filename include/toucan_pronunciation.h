/*
 * toucan_pronunciation.h - C ABI of the recording-free pronunciation check in libtoucan_hip.so (csrc/pronunciation.hip): decoding
 * the aligner's CTC posteriors (best path and prefix beam search), the Levenshtein alignment of the decoded phonemes with the
 * intended ones, and the per-phoneme posterior scores over the forced alignment.  The reference stops at a greedy decode
 * (Aligner.label_speech); DESIGN.md section 19 holds the definition and tests/pronunciation_ref.py its float64 restatement.  The
 * numbers are the aligner's opinion: PARITY of `gop` with any toolkit's goodness of pronunciation is UNPINNED.  Same conventions as
 * toucan_compare.h: device pointers owned by the caller unless marked host, ragged packed batches, one hipStream_t per call, 0 or a
 * negative TTS_E_* code, tts_last_error(); an utterance's result depends on that utterance alone, fp32 in and fp64 inside, no
 * atomics.  The only caller is the build's own Python host (ims-toucan-prosody-variance_amd/pronunciation.py, via ctypes:
 * capi.PRONUNCIATION_PROTOTYPES).
 */
#ifndef TOUCAN_PRONUNCIATION_H
#define TOUCAN_PRONUNCIATION_H

#include "toucan_tts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_PRON_MAX_SYMBOLS 256      /* columns of the logits that are symbols */
#define TTS_BEAM_MAX 32               /* widest beam of tts_ctc_beam_search */
#define TTS_CTC_SCAN_BLOCK 256        /* frames per block of the decoders' scan */
#define TTS_EDIT_MAX_REF 2048         /* reference tokens of a pair (TTS_CTC_MAX_TARGETS of toucan_score.h) */
#define TTS_EDIT_MAX_HYP 4096         /* hypothesis tokens of a pair */
#define TTS_EDIT_LDS_BP_BYTES 28672   /* the most back-pointer bytes of a pair that tts_edit_distance keeps in LDS */
#define TTS_PHONE_COLUMNS 4           /* columns of tts_phone_posteriors: mean log-posterior, gop, frame accuracy, frames */

/* One utterance of a ragged batch: the rows frame_begin ... (n_frames >= 1 of them) of the logits.  Everything that is as long as
 * the frames (hyp_id, hyp_first, hyp_last, hyp_conf, hyp_to_ref) keeps the utterance's entries at frame_begin too.  ref_begin /
 * n_ref: for tts_edit_distance the reference ids (and ref_to_hyp), for tts_phone_posteriors the full-text tokens (durations, ids,
 * and the output rows); the decoders do not read them.  scratch_off: tts_ctc_beam_search - the first 32-bit word of the history
 * table (2 n_frames beam words); tts_edit_distance - the first byte of the back-pointers (a multiple of 4), or negative to keep
 * them in LDS; otherwise not read. */
typedef struct TtsPronUtt {
  int32_t frame_begin, n_frames, ref_begin, n_ref;
  int64_t scratch_off;
} TtsPronUtt;

/* Greedy decode, one workgroup per utterance.  Per frame the argmax over the raw fp32 logits (strict >: the lowest index wins a tie)
 * and logp = x_best - max - log sum_c exp(x_c - max) in fp64 (c in index order), rounded once to fp32.  drop (uint8 [n_symbols] or
 * NULL): a frame whose argmax is a dropped symbol counts as blank.  Frame t opens a run when its symbol is not blank and differs
 * from frame t - 1's.  Out, at the front of the utterance's slots: hyp_id, hyp_first, hyp_last (frames relative to the utterance),
 * hyp_conf (the mean of logp over the run: an fp64 sum in frame order, one rounding), and n_hyp [n_utts].  An utterance that holds
 * a logit that is not finite gets n_hyp = -1 and nothing else.  utts_host [n_utts] (HOST memory) is checked here - frames outside
 * logits [rows][ld >= n_symbols] are TTS_E_ARG with a text naming the utterance - and copied to utts_dev [n_utts] on the stream. */
int tts_ctc_best_path(const float* logits, int32_t rows, int32_t ld, int32_t n_symbols, int32_t blank, const uint8_t* drop,
                      const TtsPronUtt* utts_host, TtsPronUtt* utts_dev, int32_t n_utts, int32_t* hyp_id, int32_t* hyp_first,
                      int32_t* hyp_last, float* hyp_conf, int32_t* n_hyp, tts_stream_t stream);

/* CTC prefix beam search without a language model, one workgroup per utterance, beam = 1 .. TTS_BEAM_MAX.  lp[t][c] = (x_c - max) -
 * log sum exp(x - max) in fp64.  A beam is a prefix with (pb, pnb); the search starts from the empty prefix with (0, -inf).  Per
 * frame a live beam i with last symbol e yields the stay candidate (logaddexp(pb, pnb) + lp[blank], pnb + lp[e]) and, for every
 * symbol c that is neither blank nor dropped, the extend candidate (-inf, (c == e ? pb : logaddexp(pb, pnb)) + lp[c]); an extend
 * candidate whose prefix is a live beam j is joined into j's stay candidate (pnb, by logaddexp) instead.  The next beams are the
 * `beam` candidates with the largest finite total logaddexp(pb', pnb'), a tie going to the smaller q = i (n_symbols + 1) + (0 for
 * stay, 1 + c for extend), ordered by descending total, then ascending q.  scratch [scratch_words] holds every utterance's history
 * table, two int32 (parent, symbol) per node, n_frames beam nodes, at its scratch_off; a node is made whenever an extend candidate
 * is selected, so a prefix that is pruned and made again owns several, and whether a candidate's prefix is a live beam is decided by
 * what the two spell (length, a hash, then the chains symbol by symbol), never by node numbers alone.  Out: the best prefix's ids at the front of
 * the utterance's slot of hyp_id, n_hyp [n_utts], score [n_utts] (its total, fp64); a logit that is not finite gives n_hyp = -1. */
int tts_ctc_beam_search(const float* logits, int32_t rows, int32_t ld, int32_t n_symbols, int32_t blank, const uint8_t* drop,
                        const TtsPronUtt* utts_host, TtsPronUtt* utts_dev, int32_t n_utts, int32_t beam, int32_t* scratch,
                        int64_t scratch_words, int32_t* hyp_id, int32_t* n_hyp, double* score, tts_stream_t stream);

/* Levenshtein alignment of every pair, one workgroup each: the reference ids ref_ids [n_ref_total] at ref_begin (n_ref <=
 * TTS_EDIT_MAX_REF) against the hypothesis a decoder left in hyp_id [rows] at frame_begin, n_hyp [n_utts] read on the device.
 * D(i, 0) = i, D(0, j) = j, D(i, j) = min(D(i-1, j-1) + [ref_i != hyp_j], D(i-1, j) + 1, D(i, j-1) + 1), the predecessor taken with
 * strict < in the order diagonal, deletion (i-1, j), insertion (i, j-1).  2-bit back-pointers in rows of (n_hyp + 15) / 16 words, in
 * LDS (scratch_off < 0; lds_bp_bytes <= TTS_EDIT_LDS_BP_BYTES, a multiple of 16) or at scratch + scratch_off; the host sizes the
 * slot for min(n_frames, TTS_EDIT_MAX_HYP) hypothesis tokens, and a slot that fits neither is TTS_E_ARG.  Out: counts [n_utts][4] =
 * (hits, substitutions, deletions, insertions), ref_to_hyp [n_ref_total] (the hypothesis index a reference token is matched with, -1
 * when it was deleted), hyp_to_ref [rows] (likewise, -1 for an insertion).  A pair whose n_hyp is negative or above that bound
 * gets counts of -1 and no maps. */
int tts_edit_distance(const int32_t* ref_ids, int32_t n_ref_total, const int32_t* hyp_id, int32_t rows, const int32_t* n_hyp,
                      const TtsPronUtt* utts_host, TtsPronUtt* utts_dev, int32_t n_utts, uint8_t* scratch, int64_t scratch_bytes,
                      int32_t lds_bp_bytes, int32_t* counts, int32_t* ref_to_hyp, int32_t* hyp_to_ref, tts_stream_t stream);

/* Posterior scores over the forced alignment, one workgroup per utterance: token k of the n_ref full-text tokens at ref_begin
 * owns the frames [sum_{<k} d, sum_{<k} d + d_k), d = durations (as tts_mas_durations wrote them), token_ids its symbol or -1 for
 * a word boundary.  out [n_tokens_total][4] = (mean_t lp[t][id], mean_t (lp[t][id] - max_c lp[t][c]), the share of its frames
 * whose raw argmax is id, d_k): fp64 sums in frame order, one rounding to fp32.  A token with d_k = 0 or an id outside 0 ..
 * n_symbols - 1 gets three NaN and its duration; an utterance whose durations hold a negative value or do not add up to n_frames
 * gets NaN throughout. */
int tts_phone_posteriors(const float* logits, int32_t rows, int32_t ld, int32_t n_symbols, const int32_t* durations,
                         const int32_t* token_ids, int32_t n_tokens_total, const TtsPronUtt* utts_host, TtsPronUtt* utts_dev,
                         int32_t n_utts, float* out, tts_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TOUCAN_PRONUNCIATION_H */
