"""Is a synthesised utterance still speech that says the sentence - without a recording to compare with?  The aligner's CTC posteriors
of the waveform are decoded (greedy best path, or a CTC prefix beam search), the decoded phonemes are aligned with the intended ones
(Levenshtein: phoneme error rate, and which phoneme was substituted, deleted or inserted), and every phoneme of the text gets its
mean log-posterior, goodness of pronunciation and frame accuracy over the forced alignment (tts_mas_durations), for a ragged batch
on the GPU (csrc/pronunciation.hip, include/toucan_pronunciation.h).  DESIGN.md section 19 holds the definition and the decisions,
tests/pronunciation_ref.py its float64 restatement.

The numbers are the aligner's opinion of the audio.  They are meant for comparing settings of ONE sentence against each other - a
``synthesize_grid`` sweep, an emphasis sweep - not as an absolute intelligibility score: the phoneme error rate of this small aligner
on real speech is unmeasured with either decoder, and the agreement of ``gop`` with any toolkit's GOP is UNPINNED.

The front ends are the project's own: resample.Resampler to 16 kHz and the division by the peak (compare.waves_to_16k, the route of
compare.SpeechComparator), the log-mel and the aligner of align.ProsodyExtractor, scorer.ctc_loss_batch.

Every launch computes an utterance in an order that depends on that utterance alone: a batch returns bit for bit what its
utterances return one by one.

The module-level functions need no GPU.
"""
import numpy as np
import torch

from . import align, capi
from .ragged import begins, plan_bp_store

SR = 16000
BLANK = 144  # Aligner.py:60: CTCLoss(blank=144, zero_infinity=True)
N_SYMBOLS = align.N_SYMBOLS
BEAM_MAX = capi.BEAM_MAX
MAX_REF = capi.CTC_MAX_TARGETS
MAX_HYP = capi.EDIT_MAX_HYP
LDS_BP_BYTES = capi.EDIT_LDS_BP_BYTES
SCAN_BLOCK = capi.CTC_SCAN_BLOCK
PHONE_COLUMNS = ("log_posterior", "gop", "frame_accuracy", "durations")  # the columns of tts_phone_posteriors
_ID_TO_PHONE = None


def id_to_phone():
    """dict aligner id -> symbol, the inverse of ``align.phone_ids()``; where several symbols share an id the first in sorted order
    wins (the choice align._key_to_id makes)."""
    global _ID_TO_PHONE
    if _ID_TO_PHONE is None:
        ids = align.phone_ids()
        _ID_TO_PHONE = {}
        for sym in sorted(ids):
            _ID_TO_PHONE.setdefault(int(ids[sym]), sym)
    return _ID_TO_PHONE


def check_beam(beam):
    """ValueError unless beam is an integer 0 .. BEAM_MAX (0: the greedy best path)."""
    if isinstance(beam, bool) or not isinstance(beam, (int, np.integer)) or not 0 <= beam <= BEAM_MAX:
        raise ValueError(f"beam is an integer from 0 (the greedy best path) to {BEAM_MAX}, not {beam!r}")
    return int(beam)


def drop_mask(ignore_ids, n_symbols=N_SYMBOLS, blank=BLANK):
    """uint8 [n_symbols] with a 1 at every ignored id, or None without any; ValueError for the blank or an id that is no symbol."""
    ignore = sorted({int(i) for i in ignore_ids})
    if not ignore:
        return None
    mask = np.zeros(n_symbols, dtype=np.uint8)
    for i in ignore:
        if i == blank:
            raise ValueError(f"ignore_ids holds {i}, the blank: the decoders need it")
        if not 0 <= i < n_symbols:
            raise ValueError(f"ignore_ids holds {i}, which is none of the {n_symbols} symbols")
        mask[i] = 1
    return mask


def reference_tokens(feats, ignore_ids=()):
    """[L, 62] features -> (ids of all tokens that are not word boundaries, flags [L] (align.token_ids), full_ids int32 [L]: the id
    of every full-text token, -1 at a word boundary, ref int32: the ids the edit distance compares - without the ignored ones -,
    ref_tokens int32: the full-text index of each of them, the map back)."""
    ids, flags = align.token_ids(feats)
    full_ids = np.full(len(flags), -1, dtype=np.int32)
    full_ids[(flags & 1) == 0] = ids
    ignore = {int(i) for i in ignore_ids}
    ref_tokens = np.asarray([k for k, i in enumerate(full_ids) if i >= 0 and int(i) not in ignore], dtype=np.int32)
    return ids, flags, full_ids, full_ids[ref_tokens].astype(np.int32), ref_tokens


def bp_bytes(n_ref, n_frames):
    """Bytes of back-pointers the host reserves for a pair: 2 bits per cell, rows of whole words, for as many hypothesis tokens as
    the utterance has frames (a hypothesis is never longer), at most MAX_HYP."""
    return 4 * int(n_ref) * ((min(int(n_frames), MAX_HYP) + 15) // 16)


def summarise(counts, n_ref, posteriors):
    """counts (hits, substitutions, deletions, insertions; -1 throughout when the decode failed) and the [L, 4] rows of
    tts_phone_posteriors -> the scalar entries of a result: per = (S + D + I) / max(n_ref, 1) (NaN for a failed decode), gop_mean
    over the tokens that have a gop, gop_min and gop_argmin (the full-text token; NaN and -1 when no token has one)."""
    h, s, d, i = (int(v) for v in counts)
    out = {"hits": h, "substitutions": s, "deletions": d, "insertions": i, "n_ref": int(n_ref)}
    out["per"] = float("nan") if h < 0 else (s + d + i) / max(int(n_ref), 1)
    gop = np.asarray(posteriors, dtype=np.float32).reshape(-1, len(PHONE_COLUMNS))[:, 1]
    have = np.nonzero(~np.isnan(gop))[0]
    if len(have):
        k = int(have[np.argmin(gop[have])])
        out.update(gop_mean=float(gop[have].astype(np.float64).mean()), gop_min=float(gop[k]), gop_argmin=k)
    else:
        out.update(gop_mean=float("nan"), gop_min=float("nan"), gop_argmin=-1)
    return out


class PronunciationChecker:
    """``check(texts, waves, sr)``: one dict per utterance (below); ``recognise`` decodes only; ``check_logits`` starts from given
    posteriors; ``best_path``, ``beam_search``, ``edit_distance`` and ``phone_posteriors`` are the four kernels on their own."""

    def __init__(self, aligner_state_dict=None, device=None, extractor=None):
        """extractor: a cloner's align.ProsodyExtractor to share (the aligner is packed once), else one is built from the
        reference-schema state dict on ``device`` (capi.ToucanHipError for a CPU device)."""
        if extractor is None:
            if aligner_state_dict is None or device is None:
                raise ValueError("PronunciationChecker takes an aligner state dict and a device, or extractor=")
            extractor = align.ProsodyExtractor(aligner_state_dict, device)
        self.extractor = extractor
        self.aligner = extractor.aligner
        self.ops = extractor.ops
        self.device = extractor.device
        self._resampler = None

    # ---- the kernels ------------------------------------------------------------------------------------------------------
    def _i32(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    def _table(self, rag, ref_counts=None, scratch_off=None):
        B = rag.n_seq
        table = (capi.TtsPronUtt * max(B, 1))()
        rb = begins(ref_counts) if ref_counts is not None else [0] * B
        for b in range(B):
            table[b] = capi.TtsPronUtt(int(rag.begins[b]), int(rag.lengths[b]), rb[b], 0 if ref_counts is None else int(ref_counts[b]),
                                       -1 if scratch_off is None else int(scratch_off[b]))
        return table, torch.empty(max(B, 1) * 24, dtype=torch.uint8, device=self.device)

    def _check_logits_tensor(self, logits, n_symbols):
        assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and logits.device == self.device, \
            f"float32 logits [rows, ld] on {self.device}"
        if not 1 <= n_symbols <= logits.shape[1]:
            raise ValueError(f"{n_symbols} symbols in logits of {logits.shape[1]} columns")

    def _drop(self, drop):
        return None if drop is None else torch.from_numpy(np.ascontiguousarray(drop, dtype=np.uint8)).to(self.device)

    def best_path(self, logits, rag, n_symbols=N_SYMBOLS, blank=BLANK, drop=None):
        """-> dict of device tensors: hyp_id, hyp_first, hyp_last (int32 [rows]), hyp_conf (float32 [rows]), every utterance's
        entries at the front of its frames, and n_hyp (int32 [B], -1 for a logit that is not finite)."""
        self._check_logits_tensor(logits, n_symbols)
        ops, rows, B = self.ops, int(logits.shape[0]), rag.n_seq
        table, dev = self._table(rag)
        out = {k: torch.zeros(max(rows, 1), dtype=torch.int32, device=self.device) for k in ("hyp_id", "hyp_first", "hyp_last")}
        out["hyp_conf"] = torch.zeros(max(rows, 1), dtype=torch.float32, device=self.device)
        out["n_hyp"] = torch.zeros(max(B, 1), dtype=torch.int32, device=self.device)
        d = self._drop(drop)
        capi.check(ops.lib.tts_ctc_best_path(logits.data_ptr(), rows, int(logits.stride(0)), int(n_symbols), int(blank), None if d is None else d.data_ptr(),
                                             table, dev.data_ptr(), B, out["hyp_id"].data_ptr(), out["hyp_first"].data_ptr(), out["hyp_last"].data_ptr(),
                                             out["hyp_conf"].data_ptr(), out["n_hyp"].data_ptr(), ops.stream()), "tts_ctc_best_path")
        out["n_hyp"] = out["n_hyp"][:B]
        return out

    def beam_search(self, logits, rag, beam, n_symbols=N_SYMBOLS, blank=BLANK, drop=None):
        """-> dict of device tensors: hyp_id (int32 [rows]), n_hyp (int32 [B]), score (float64 [B])."""
        self._check_logits_tensor(logits, n_symbols)
        beam = check_beam(beam)
        if beam < 1:
            raise ValueError("the beam search needs a beam of at least 1")
        ops, rows, B = self.ops, int(logits.shape[0]), rag.n_seq
        words = [2 * n * beam for n in rag.lengths]
        table, dev = self._table(rag, scratch_off=begins(words))
        scratch = torch.empty(max(sum(words), 1), dtype=torch.int32, device=self.device)
        out = {"hyp_id": torch.zeros(max(rows, 1), dtype=torch.int32, device=self.device),
               "n_hyp": torch.zeros(max(B, 1), dtype=torch.int32, device=self.device),
               "score": torch.zeros(max(B, 1), dtype=torch.float64, device=self.device)}
        d = self._drop(drop)
        capi.check(ops.lib.tts_ctc_beam_search(logits.data_ptr(), rows, int(logits.stride(0)), int(n_symbols), int(blank), None if d is None else d.data_ptr(),
                                               table, dev.data_ptr(), B, beam, scratch.data_ptr(), int(sum(words)), out["hyp_id"].data_ptr(),
                                               out["n_hyp"].data_ptr(), out["score"].data_ptr(), ops.stream()), "tts_ctc_beam_search")
        out["n_hyp"], out["score"] = out["n_hyp"][:B], out["score"][:B]
        return out

    def edit_distance(self, refs, hyp_id, n_hyp, rag, force_scratch=False, fill=-1):
        """refs: per utterance its reference ids; hyp_id / n_hyp: what a decoder left on the device.  -> (counts int32 [B, 4],
        ref_to_hyp int32 [sum of the references], hyp_to_ref int32 [rows]) on the device.  force_scratch: every pair keeps its
        back-pointers in the scratch buffer, whatever its size (tests).  fill: what both maps hold before the launch - the kernel
        writes every token of a pair it aligns and nothing of a pair whose decode failed."""
        ops, B, rows = self.ops, rag.n_seq, int(hyp_id.numel())
        n_ref = [len(r) for r in refs]
        if len(refs) != B:
            raise ValueError(f"{len(refs)} references for {B} utterances")
        for b, n in enumerate(n_ref):
            if n > MAX_REF:
                raise ValueError(f"utterance {b}: {n} reference tokens; the edit distance takes at most {MAX_REF}")
        off, total, lds = plan_bp_store([bp_bytes(n, T) for n, T in zip(n_ref, rag.lengths)], LDS_BP_BYTES, force_scratch)
        table, dev = self._table(rag, ref_counts=n_ref, scratch_off=off)
        scratch = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        ids = self._i32(np.concatenate([np.asarray(r, dtype=np.int32).reshape(-1) for r in refs] + [np.zeros(1, dtype=np.int32)]))
        counts = torch.zeros(max(B, 1), 4, dtype=torch.int32, device=self.device)
        r2h = torch.full((max(sum(n_ref), 1),), int(fill), dtype=torch.int32, device=self.device)
        h2r = torch.full((max(rows, 1),), int(fill), dtype=torch.int32, device=self.device)
        capi.check(ops.lib.tts_edit_distance(ids.data_ptr(), int(sum(n_ref)), hyp_id.data_ptr(), rows, n_hyp.data_ptr(), table, dev.data_ptr(), B,
                                             scratch.data_ptr(), total, lds, counts.data_ptr(), r2h.data_ptr(), h2r.data_ptr(),
                                             ops.stream()), "tts_edit_distance")
        return counts[:B], r2h[:sum(n_ref)], h2r

    def phone_posteriors(self, logits, rag, durations, full_ids, n_symbols=N_SYMBOLS):
        """durations: int32 on the device, the full texts packed (AlignerEngine.durations); full_ids: per utterance the id of every
        full-text token, -1 at a word boundary.  -> float32 [sum of tokens, 4] on the device, columns PHONE_COLUMNS."""
        self._check_logits_tensor(logits, n_symbols)
        ops, B = self.ops, rag.n_seq
        n_full = [len(f) for f in full_ids]
        total = int(sum(n_full))
        assert durations.dtype == torch.int32 and durations.numel() == total, f"{durations.numel()} durations for {total} tokens"
        table, dev = self._table(rag, ref_counts=n_full)
        ids = self._i32(np.concatenate([np.asarray(f, dtype=np.int32).reshape(-1) for f in full_ids] + [np.zeros(1, dtype=np.int32)]))
        dur = durations if total else torch.zeros(1, dtype=torch.int32, device=self.device)
        out = torch.zeros(max(total, 1), len(PHONE_COLUMNS), dtype=torch.float32, device=self.device)
        capi.check(ops.lib.tts_phone_posteriors(logits.data_ptr(), int(logits.shape[0]), int(logits.stride(0)), int(n_symbols), dur.data_ptr(),
                                                ids.data_ptr(), total, table, dev.data_ptr(), B, out.data_ptr(), ops.stream()), "tts_phone_posteriors")
        return out[:total]

    # ---- decode --------------------------------------------------------------------------------------------------------------
    def _decode(self, logits, rag, beam, drop):
        return self.best_path(logits, rag, drop=drop) if beam == 0 else self.beam_search(logits, rag, beam, drop=drop)

    def _hypotheses(self, dec, rag, beam):
        """The decoders' device tensors -> per utterance the dict entries of its hypothesis (one copy to the host each)."""
        host = {k: v.cpu().numpy() for k, v in dec.items()}
        names = id_to_phone()
        out = []
        for b, (b0, _) in enumerate(zip(rag.begins, rag.lengths)):
            n = int(host["n_hyp"][b])
            m = max(n, 0)
            r = {"n_hyp": n, "hyp_ids": host["hyp_id"][b0:b0 + m].copy()}
            r["hyp_phones"] = [names.get(int(i), "?") for i in r["hyp_ids"]]
            if beam == 0:
                r.update(hyp_first=host["hyp_first"][b0:b0 + m].copy(), hyp_last=host["hyp_last"][b0:b0 + m].copy(),
                         hyp_conf=host["hyp_conf"][b0:b0 + m].copy())
            else:
                r["beam_score"] = float(host["score"][b]) if n >= 0 else float("nan")
            out.append(r)
        return out

    @torch.inference_mode()
    def check_logits(self, logits, rag, feats, beam=8, ignore_ids=()):
        """logits: float32 [rows, 145] on the device laid out by ``rag`` (AlignerEngine.logits); feats: per utterance its [L, 62]
        features.  -> one dict per utterance:
          per = (S + D + I) / max(n_ref, 1), hits, substitutions, deletions, insertions, n_ref, n_hyp
          hyp_ids, hyp_phones: the decoded phonemes (``ignore_ids`` left out, as they are from the reference)
          ref_tokens: the full-text index of every reference token; ref_to_hyp [L]: the hypothesis index a full-text token is matched
          with (hit or substitution), -1 when it was deleted or is no reference token; hyp_to_ref: the full-text token a decoded
          phoneme is matched with, -1 for an insertion
          beam_score (the best prefix's log-probability), or with beam=0 hyp_first / hyp_last / hyp_conf: the frames of every run
          of the best path and the mean log-posterior over them
          ctc_loss: scorer.ctc_loss_batch of the whole reference
          durations, log_posterior, gop, frame_accuracy [L]: the forced alignment's frames per full-text token, the mean
          log-posterior of the token's symbol over them, the mean of its distance to the frame's best symbol (never positive), the
          share of its frames whose best symbol it is; NaN for word boundaries and tokens without a frame
          gop_mean, gop_min, gop_argmin (``summarise``).
        ValueError, naming the utterance, for lists of unequal length, a text without a phoneme, a reference longer than MAX_REF, a
        beam outside 0 .. BEAM_MAX and an ignored id that is the blank."""
        from . import scorer
        beam = check_beam(beam)
        drop = drop_mask(ignore_ids)
        if len(feats) != rag.n_seq:
            raise ValueError(f"{len(feats)} texts for {rag.n_seq} utterances")
        toks = []
        for b, f in enumerate(feats):
            try:
                toks.append(reference_tokens(f, ignore_ids))
            except ValueError as e:
                raise ValueError(f"utterance {b}: {e}") from e
            if len(toks[-1][0]) == 0:
                raise ValueError(f"utterance {b}: its text holds no phoneme")
            if len(toks[-1][0]) > MAX_REF:
                raise ValueError(f"utterance {b}: {len(toks[-1][0])} aligner tokens; the CTC kernels take at most {MAX_REF}")
        if rag.n_seq == 0:
            return []
        self._check_logits_tensor(logits, N_SYMBOLS)
        if logits.shape[1] != N_SYMBOLS or not logits.is_contiguous():
            raise ValueError(f"check_logits takes contiguous logits of {N_SYMBOLS} columns")
        ids, flags = [t[0] for t in toks], [t[1] for t in toks]
        dec = self._decode(logits, rag, beam, drop)
        counts, r2h, h2r = self.edit_distance([t[3] for t in toks], dec["hyp_id"], dec["n_hyp"], rag)
        loss = scorer.ctc_loss_batch(self.ops, logits, rag, ids, blank=BLANK)
        dur, full_begin = self.aligner.durations(logits, rag, ids, flags)
        post = self.phone_posteriors(logits, rag, dur, [t[2] for t in toks])
        results = self._hypotheses(dec, rag, beam)
        counts, r2h, h2r, loss, post, dur = (t.cpu().numpy() for t in (counts, r2h, h2r, loss, post, dur))
        rb = begins([len(t[3]) for t in toks])
        for b, (r, t) in enumerate(zip(results, toks)):
            L, ref_tokens, n_ref = len(t[1]), t[4], len(t[3])
            rows = post[full_begin[b]:full_begin[b] + L]
            r.update(summarise(counts[b], n_ref, rows))
            full_r2h = np.full(L, -1, dtype=np.int32)
            m = max(r["n_hyp"], 0)
            back = np.full(m, -1, dtype=np.int32)
            if r["n_hyp"] >= 0:
                full_r2h[ref_tokens] = r2h[rb[b]:rb[b] + n_ref]
                raw = h2r[rag.begins[b]:rag.begins[b] + m]
                back[raw >= 0] = ref_tokens[raw[raw >= 0]]
            r.update(ref_tokens=ref_tokens, ref_to_hyp=full_r2h, hyp_to_ref=back, ctc_loss=float(loss[b]),
                     durations=dur[full_begin[b]:full_begin[b] + L].copy(), log_posterior=rows[:, 0].copy(), gop=rows[:, 1].copy(),
                     frame_accuracy=rows[:, 2].copy())
        return results

    # ---- waves ---------------------------------------------------------------------------------------------------------------
    def _logits_of(self, waves, sr):
        from . import compare
        B = len(waves)
        srs = [int(s) for s in sr] if isinstance(sr, (list, tuple)) else [int(sr)] * B
        if len(srs) != B:
            raise ValueError(f"{len(srs)} sample rates for {B} waves")
        w16 = compare.waves_to_16k(self, waves, srs, [f"utterance {b}" for b in range(B)])
        ext = self.extractor
        spec, rag = ext.spectra(w16)
        return self.aligner.logits(ext.log_mel(spec, rag), rag), rag

    @torch.inference_mode()
    def check(self, texts, waves, sr, beam=8, ignore_ids=()):
        """texts: phoneme strings or [L, 62] features; waves: mono waves at ``sr`` (one rate, or one per wave), brought to 16 kHz by
        the device resampler and divided by their peaks (compare.waves_to_16k), then the log-mel and the aligner of the extractor,
        then ``check_logits`` (which documents the result).  ValueError, naming the utterance, also for a sample that is not finite
        and a wave too short for the STFT."""
        from .phonemes import phones_to_features
        beam = check_beam(beam)
        drop_mask(ignore_ids)
        if len(texts) != len(waves):
            raise ValueError(f"{len(texts)} texts for {len(waves)} waves")
        feats = [phones_to_features(t, handle_missing=False) if isinstance(t, str) else np.asarray(t, dtype=np.float32) for t in texts]
        for b, f in enumerate(feats):  # (before the first launch)
            n = int((np.asarray(f)[:, align.IDX["word_boundary"]] == 0).sum())
            if n == 0:
                raise ValueError(f"utterance {b}: its text holds no phoneme")
            if n > MAX_REF:
                raise ValueError(f"utterance {b}: {n} aligner tokens; the CTC kernels take at most {MAX_REF}")
        if len(texts) == 0:
            return []
        logits, rag = self._logits_of(waves, sr)
        return self.check_logits(logits, rag, feats, beam=beam, ignore_ids=ignore_ids)

    @torch.inference_mode()
    def recognise(self, waves, sr, beam=8, ignore_ids=()):
        """Decode only -> per wave n_hyp, hyp_ids, hyp_phones and beam_score, or with beam=0 hyp_first / hyp_last / hyp_conf."""
        beam = check_beam(beam)
        drop = drop_mask(ignore_ids)
        if len(waves) == 0:
            return []
        logits, rag = self._logits_of(waves, sr)
        return self._hypotheses(self._decode(logits, rag, beam, drop), rag, beam)
