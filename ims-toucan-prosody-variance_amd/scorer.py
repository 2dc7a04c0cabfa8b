"""Drop-in counterpart of the reference's Utility/Scorer.py on the HIP kernels: score every utterance of a corpus cache to find
problematic samples.

* ``AlignmentScorer`` (:24-76): the aligner's CTC loss per utterance of ``aligner_train_cache.pt`` (a high loss flags a mislabelled
  transcript).  Logits: ``align.AlignerEngine.logits``; the loss: ``tts_ctc_loss`` (csrc/score.hip).
* ``TTSScorer`` (:79-199): the acoustic model's teacher-forced loss per utterance of ``fast_train_cache.pt`` (a high loss flags bad
  audio), and the removal of the worst samples from the cache.  Style embedding: ``style.StyleEngine``; forward pass: the stage API
  (``tts_encoder``, ``tts_teacher_forced``, ``tts_decoder``, ``tts_postnet``); the four losses: ``tts_score_losses``.  On request
  (``score(..., include_glow=True)``) the fifth loss of ``ToucanTTS.forward``, which the reference's scorer leaves out
  (``run_glow=False``): the negative log-likelihood of the gold spectrogram under the PostFlow, ``tts_postflow_nll``.

Both score ragged batches of utterances sorted by length (``score(..., batch_size=32)``, an additive argument); results are per file
path, in the cache's order.  An utterance's score does not depend on its batch: bit for bit for the CTC loss, to rounding order for
the acoustic losses (the frame stages' tile forms depend on the grid).

Deviations from the reference: the models score in eval mode (the reference never calls ``.eval()``, so its own
scores carry dropout and batch-of-one BatchNorm statistics); fp32 only; caches are read, never built (building one needs aligner
fine-tuning and Praat pitch); ``remove_samples_with_highest_loss`` removes an index that is both a NaN and among the worst once.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import align, capi, native, style
from .interface import MODELS_DIR, _load_checkpoint, _to_numpy_sd
from .phonemes import get_language_id
from .ragged import Ragged

BLANK = 144  # Aligner.py:60: CTCLoss(blank=144, zero_infinity=True)
ALIGNER_CACHE, TTS_CACHE = "aligner_train_cache.pt", "fast_train_cache.pt"


# ---- caches ------------------------------------------------------------------------------------------------------------------
def read_aligner_cache(path):
    """aligner_train_cache.pt (AlignerDataset.py:109: ``(datapoints, norm_waves, speaker_embeddings, filepaths)``, a datapoint being
    ``[text [L, 62], text_len, mel [T, 80], mel_len]``) -> (list of (text, mel) numpy pairs, file paths).  ``path`` may also name the
    corpus directory."""
    if os.path.isdir(path):
        path = os.path.join(path, ALIGNER_CACHE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: no aligner cache.  Building one (AlignerDataset) needs the reference's audio preprocessing and "
                                f"speaker embedding models, which are not available here; the scorer only reads existing caches.")
    data = torch.load(path, map_location="cpu", weights_only=True)
    datapoints, filepaths = data[0], data[3]
    items = []
    for i, dp in enumerate(datapoints):
        text = np.asarray(dp[0], dtype=np.float32)
        mel = np.asarray(dp[2], dtype=np.float32)
        if text.ndim != 2 or text.shape[1] != 62 or mel.ndim != 2 or mel.shape[1] != 80 or mel.shape[0] < 1:
            raise ValueError(f"{path}: datapoint {i}: text {text.shape} / mel {mel.shape} (expected [L, 62] / [T >= 1, 80])")
        items.append((text, mel))
    return items, list(filepaths)


def read_tts_cache(corpus_dir):
    """fast_train_cache.pt (FastSpeechDataset.py:97-105: ``[text [L, 62], text_len, spec [T, 80], spec_len, durations [L], energy [L, 1],
    pitch [L, 1], prosodic condition, filepath]`` per datapoint) -> (the raw datapoints, list of dicts of numpy arrays).  The shapes
    are checked: a [L] pitch or energy would broadcast to [1, L, L] in the reference's MSE, and the durations must add up to the
    spectrogram's frames."""
    path = os.path.join(corpus_dir, TTS_CACHE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path}: no ToucanTTS cache.  Building one (prepare_fastspeech_corpus) needs aligner fine-tuning and "
                                f"Praat pitch extraction, which are not available here; the scorer only reads existing caches.")
    datapoints = torch.load(path, map_location="cpu", weights_only=True)
    items = []
    for i, dp in enumerate(datapoints):
        text = np.asarray(dp[0], dtype=np.float32)
        spec = np.asarray(dp[2], dtype=np.float32)
        dur = np.asarray(dp[4]).astype(np.int64)
        energy, pitch = np.asarray(dp[5], dtype=np.float32), np.asarray(dp[6], dtype=np.float32)
        L = text.shape[0] if text.ndim == 2 else -1
        if text.ndim != 2 or text.shape[1] != 62 or spec.ndim != 2 or spec.shape[1] != 80:
            raise ValueError(f"{path}: datapoint {i}: text {text.shape} / spec {spec.shape} (expected [L, 62] / [T, 80])")
        if dur.shape != (L,) or pitch.shape != (L, 1) or energy.shape != (L, 1):
            raise ValueError(f"{path}: datapoint {i}: durations {dur.shape}, pitch {pitch.shape}, energy {energy.shape} "
                             f"(expected [{L}], [{L}, 1], [{L}, 1])")
        if (dur < 0).any() or int(dur.sum()) != spec.shape[0] or L < 1:
            raise ValueError(f"{path}: datapoint {i}: the durations add up to {int(dur.sum())} frames, the spectrogram has {spec.shape[0]}")
        items.append(dict(text=text, spec=spec, durations=dur, pitch=pitch.reshape(-1), energy=energy.reshape(-1), filepath=dp[8]))
    return datapoints, items


class ScoredCorpus:
    """What the reference keeps as ``current_dset`` (a FastSpeechDataset): the datapoints of the cache and ``remove_samples``
    (FastSpeechDataset.py:191-195), which pops ids in descending order and rewrites fast_train_cache.pt."""

    def __init__(self, cache_dir, datapoints, language_id):
        self.cache_dir = cache_dir
        self.datapoints = datapoints
        self.language_id = language_id

    def __len__(self):
        return len(self.datapoints)

    def remove_samples(self, list_of_samples_to_remove):
        # deviation: an id listed twice (a NaN that is also among the worst) is removed once; the reference would pop it twice and
        # lose an unrelated sample
        for remove_id in sorted(set(int(i) for i in list_of_samples_to_remove), reverse=True):
            self.datapoints.pop(remove_id)
        torch.save(self.datapoints, os.path.join(self.cache_dir, TTS_CACHE))
        print("Dataset updated!")


def _batches(lengths, batch_size):
    """Indices sorted by length (longest first, ties by index), cut into batches."""
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    return [order[k:k + batch_size] for k in range(0, len(order), batch_size)]


def _show(path_to_score, nans, n, trailing_blank):
    if len(nans) > 0:
        print("The following filepaths had an infinite loss:")
        for path in nans:
            print(path)
        print("\n\n")
    for index, path in enumerate(sorted(path_to_score, key=path_to_score.get, reverse=True)):
        if index < n or n == -1:
            print(f"Loss: {round(path_to_score[path], 3)} - Path: {path}")
    if trailing_blank:
        print("\n\n")


def _ti(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


# ---- CTC -------------------------------------------------------------------------------------------------------------------
def ctc_loss_batch(ops, logits, rag, id_lists, blank=BLANK):
    """tts_ctc_loss on logits [rows, 145] laid out by ``rag`` with one id sequence per utterance -> float32 device tensor [B]."""
    dev, B = ops.device, rag.n_seq
    n_ids = [len(i) for i in id_lists]
    if max(n_ids, default=0) > capi.CTC_MAX_TARGETS:
        raise ValueError(f"{max(n_ids)} aligner tokens in one utterance; the CTC kernel takes at most {capi.CTC_MAX_TARGETS}")
    tb = np.concatenate([[0], np.cumsum(n_ids)[:-1]]) if B else np.zeros(0)
    ids = np.concatenate([np.asarray(i, dtype=np.int32) for i in id_lists] + [np.zeros(1, dtype=np.int32)])
    fb, nf, tg, tbd, nt = _ti(rag.begins, dev), _ti(rag.lengths, dev), _ti(ids, dev), _ti(tb, dev), _ti(n_ids, dev)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    capi.check(ops.lib.tts_ctc_loss(logits.data_ptr(), int(logits.stride(0)), int(logits.shape[1]), fb.data_ptr(), nf.data_ptr(), tg.data_ptr(),
                                    tbd.data_ptr(), nt.data_ptr(), B, blank, max(n_ids, default=0), out.data_ptr(), ops.stream()), "tts_ctc_loss")
    return out


class AlignmentScorer:

    def __init__(self, path_to_aligner_model, device, timing=False):
        self.path_to_score = dict()
        self.device = device
        self.nans = list()
        sd = _load_checkpoint(path_to_aligner_model)["asr_model"]
        self.aligner = align.AlignerEngine(_to_numpy_sd(sd), device, timing=timing)
        self.timing = timing
        self.last_phase_ms = {}

    @torch.inference_mode()
    def score_items(self, items, batch_size=32):
        """items: list of (text [L, 62], mel [T, 80]) -> numpy float32 CTC losses in the items' order."""
        eng = self.aligner
        ops, dev = eng.ops, eng.device
        ids = [align.token_ids(t)[0] for t, _ in items]
        losses = np.zeros(len(items), dtype=np.float32)
        self.last_phase_ms = {}
        for batch in _batches([m.shape[0] for _, m in items], batch_size):
            mels = [items[i][1] for i in batch]
            rag = Ragged([m.shape[0] for m in mels], dev)
            x = torch.from_numpy(np.concatenate(mels)).to(dev)
            eng._mark("logits")
            lg = eng.logits(x, rag)
            eng._mark("ctc")
            out = ctc_loss_batch(ops, lg, rag, [ids[i] for i in batch])
            eng._mark("end")
            if self.timing:  # AlignerEngine.logits marks its own "convs" / "lstm" phases: they add up to "logits"
                eng._collect()
                for k, v in eng.last_phase_ms.items():
                    k = "ctc" if k == "ctc" else "logits"
                    self.last_phase_ms[k] = self.last_phase_ms.get(k, 0.0) + v
            losses[batch] = out.cpu().numpy()
        return losses

    def score(self, path_to_aligner_dataset, batch_size=32):
        """
        call this to update the path_to_score dict with scores for this dataset
        """
        items, filepaths = read_aligner_cache(path_to_aligner_dataset)
        self.nans = list()
        self.path_to_score = dict()
        losses = self.score_items(items, batch_size)
        for index, fp in enumerate(filepaths[:len(items)]):
            loss = float(losses[index])
            if math.isnan(loss):
                self.nans.append(fp)
            self.path_to_score[fp] = loss
        if len(self.nans) > 0:
            print("The following filepaths had an infinite loss:")
            for path in self.nans:
                print(path)

    def show_samples_with_highest_loss(self, n=-1):
        """
        NaN samples will always be shown.
        To see all samples, pass -1, otherwise n samples will be shown.
        """
        _show(self.path_to_score, self.nans, n, trailing_blank=False)


# ---- teacher-forced acoustic losses ------------------------------------------------------------------------------------------
class TTSScorer:

    def __init__(self,
                 path_to_model,
                 device,
                 path_to_embedding_checkpoint=os.path.join(MODELS_DIR, "Embedding", "embedding_function.pt"),
                 timing=False
                 ):
        self.device = device
        self.path_to_score = dict()
        self.path_to_id = dict()
        self.path_to_parts = dict()
        self.path_to_row_scores = dict()
        self.nans = list()
        self.nan_indexes = list()
        # the reference's fallbacks ToucanTTS(lang_embs=None) / (lang_embs=None, utt_embed_dim=None) (:95-104): the pipeline reads the
        # variant off the state dict
        weights = _to_numpy_sd(_load_checkpoint(path_to_model)["model"])
        self.pipe = native.NativePipeline(weights, None, None, device, precision="f32", scoring=True)
        self.style_embedding_function = style.StyleEngine(_to_numpy_sd(_load_checkpoint(path_to_embedding_checkpoint)["style_emb_func"]),
                                                          self.pipe.device)
        self.nans_removed = False
        self.current_dset = None
        self.timing = timing
        self.last_phase_ms = {}

    @torch.inference_mode()
    def forward_batch(self, items, lang_id, include_glow=False, keep_row_scores=False):
        """One ragged batch through the teacher-forced forward pass and the loss kernel.  items: dicts of read_tts_cache.  -> dict with
        ``losses`` [B, 4] (l1, duration, pitch, energy; device) and the device buffers of the pass (predictions, packed mels, layouts).
        include_glow: ``losses`` is [B, 5], the glow loss last (tts_postflow_nll: the PostFlow run forward on the gold mel, conditioned
        on the pass's own PostNet output; NaN for an utterance of fewer than two frames).  keep_row_scores (with include_glow):
        ``glow_rows`` is the float32 device tensor [total frames / 2, 2] of tts_glow_nll_reduce's row parts, utterance u at row
        ``rag_frame.begins[u] // 2`` with ``T // 2`` rows (``row_scores_of``)."""
        pipe = self.pipe
        dev, lib = pipe.device, pipe.lib
        with torch.cuda.device(dev):
            st = pipe._stream()
            ev = []

            def mark(name):  # HIP events between the phases (timing=True: tools/bench_score.py)
                if self.timing:
                    ev.append((name, torch.cuda.Event(enable_timing=True)))
                    ev[-1][1].record()
            B = len(items)
            Ls = [it["text"].shape[0] for it in items]
            Ts = [it["spec"].shape[0] for it in items]
            pipe._ensure_pe(max(Ls + Ts))
            embs = None
            mark("style")
            if pipe.multispeaker:
                embs = self.style_embedding_function.forward([torch.from_numpy(it["spec"]) for it in items])
            mark("acoustic")
            packed = pipe.pack_inputs([torch.from_numpy(it["text"]) for it in items], embs, [lang_id] * B,
                                      [it["durations"] for it in items], [it["pitch"] for it in items], [it["energy"] for it in items])
            ptr = native.ptr
            capi.check(lib.tts_encoder(pipe.h, ptr(packed["text"]), ptr(packed["emb"]), ptr(packed["lang"]), (C.c_int32 * B)(*Ls), B, st),
                       "tts_encoder")
            R = sum(Ls)
            pred = torch.empty(3, R, dtype=torch.float32, device=dev)  # log durations, pitch, energy
            frames = (C.c_int32 * B)()
            capi.check(lib.tts_teacher_forced(pipe.h, ptr(packed["gp"]), ptr(packed["ge"]), ptr(packed["gd"]), ptr(pred[0]), ptr(pred[1]),
                                              ptr(pred[2]), frames, st), "tts_teacher_forced")
            assert [int(f) for f in frames] == Ts, "teacher forcing: frame counts differ from the spectrograms (read_tts_cache checks this)"
            capi.check(lib.tts_decoder(pipe.h, st), "tts_decoder")
            capi.check(lib.tts_postnet(pipe.h, st), "tts_postnet")
            rag_f, rag_p = Ragged(Ts, dev, align=2), Ragged(Ls, dev)
            RF = rag_f.total_rows
            before = torch.empty(RF, 80, dtype=torch.float32, device=dev)
            capi.check(lib.tts_copy_decoder_mel(pipe.h, ptr(before), 80, st), "tts_copy_decoder_mel")
            after, ld = C.c_void_p(), C.c_int32()
            capi.check(lib.tts_mel(pipe.h, C.byref(after), C.byref(ld), None, None), "tts_mel")  # [refined | text], row stride 272
            gold_h = np.zeros((RF, 80), dtype=np.float32)
            for it, b0 in zip(items, rag_f.begins):
                gold_h[b0:b0 + it["spec"].shape[0]] = it["spec"]
            gold = torch.from_numpy(gold_h).to(dev)
            mark("loss")
            fb, nf, pb, npd = _ti(rag_f.begins, dev), _ti(Ts, dev), _ti(rag_p.begins, dev), _ti(Ls, dev)
            losses = torch.empty(B, 4, dtype=torch.float32, device=dev)
            capi.check(lib.tts_score_losses(ptr(before), 80, after, int(ld.value), ptr(gold), 80, ptr(fb), ptr(nf), ptr(pred[0]), ptr(pred[1]),
                                            ptr(pred[2]), ptr(packed["gd"]), ptr(packed["gp"]), ptr(packed["ge"]), ptr(pb), ptr(npd), B,
                                            ptr(losses), st), "tts_score_losses")
            glow_rows = None
            if include_glow:
                mark("glow")
                glow = torch.empty(B, dtype=torch.float32, device=dev)
                if keep_row_scores:
                    glow_rows = torch.zeros(RF // 2, 2, dtype=torch.float32, device=dev)
                capi.check(lib.tts_postflow_nll(pipe.h, ptr(gold), 80, ptr(glow), ptr(glow_rows), None, st), "tts_postflow_nll")
                losses = torch.cat([losses, glow[:, None]], dim=1)
            mark("end")
            if ev:
                torch.cuda.synchronize(dev)
                for (name, e0), (_, e1) in zip(ev[:-1], ev[1:]):
                    self.last_phase_ms[name] = self.last_phase_ms.get(name, 0.0) + e0.elapsed_time(e1)
            return dict(losses=losses, pred=pred, before=before, gold=gold, rag_frame=rag_f, rag_phone=rag_p, packed=packed, glow_rows=glow_rows)

    @staticmethod
    def row_scores_of(out, index):
        """The row parts [T // 2, 2] (numpy float32) of utterance ``index`` of a forward_batch(..., keep_row_scores=True) result."""
        rag = out["rag_frame"]
        r0, n = int(rag.begins[index]) // 2, int(rag.lengths[index]) // 2
        return out["glow_rows"][r0:r0 + n].cpu().numpy()

    def score_items(self, items, lang_id, batch_size=32, include_glow=False, keep_row_scores=False):
        """items: dicts of read_tts_cache -> numpy float32 [n, 4] losses (l1, duration, pitch, energy) in the items' order; with
        include_glow [n, 5], the glow loss last.  keep_row_scores (with include_glow): ``self.last_row_scores`` is the list of the
        items' row parts, each float32 [T // 2, 2] (see ``score``)."""
        out = np.zeros((len(items), 5 if include_glow else 4), dtype=np.float32)
        self.last_phase_ms = {}
        self.last_row_scores = [None] * len(items) if include_glow and keep_row_scores else None
        for batch in _batches([it["spec"].shape[0] for it in items], batch_size):
            if not include_glow:
                out[batch] = self.forward_batch([items[i] for i in batch], lang_id)["losses"].cpu().numpy()
                continue
            res = self.forward_batch([items[i] for i in batch], lang_id, include_glow=True, keep_row_scores=keep_row_scores)
            out[batch] = res["losses"].cpu().numpy()
            if self.last_row_scores is not None:
                for k, i in enumerate(batch):
                    self.last_row_scores[i] = self.row_scores_of(res, k)
        return out

    def score(self, path_to_toucantts_dataset, lang_id, batch_size=32, include_glow=False, keep_row_scores=False):
        """
        call this to update the path_to_score dict with scores for this dataset

        include_glow: the score is l1 + duration + pitch + energy + glow, the five losses of the reference's ``ToucanTTS.forward``
        with ``run_glow=True`` (its own scorer passes ``run_glow=False``), and ``path_to_parts[filepath]`` holds the five values.  The
        glow loss is the negative log-likelihood per spectrogram bin of the gold spectrogram under the PostFlow; it reacts to clicks,
        clipping and noise bursts that the l1 average smooths over.

        keep_row_scores (with include_glow): ``path_to_row_scores[filepath]`` is a float32 array [T // 2, 2]; row r covers the frames
        2r and 2r + 1 (an odd last frame belongs to no row: the flow's squeeze drops it).  Column 0 is the row's prior term,
        sum over its 160 latent values of z^2 / 2 + log(2 pi) / 2; column 1 is the row's log-determinant.  They add up to the loss as
        ``glow = rows[:, 0].sum() / (160 * (T // 2)) - rows[:, 1].sum() / (80 * T)``: a row whose column 0 is large, or whose column 1
        is small, is where the file is unlikely.
        """
        lid = get_language_id(lang_id)
        if lid is None:
            raise ValueError(f"language {lang_id!r} has no id (Preprocessing/TextFrontend.py:490-524)")
        if keep_row_scores and not include_glow:
            raise ValueError("keep_row_scores=True needs include_glow=True: the row scores are the parts of the glow loss")
        datapoints, items = read_tts_cache(path_to_toucantts_dataset)
        parts = self.score_items(items, lid, batch_size, include_glow=include_glow, keep_row_scores=keep_row_scores)
        self.record_scores(ScoredCorpus(path_to_toucantts_dataset, datapoints, lid), items, parts, include_glow=include_glow)
        self.path_to_row_scores = dict()
        if keep_row_scores:
            self.path_to_row_scores = {it["filepath"]: rows for it, rows in zip(items, self.last_row_scores)}

    def record_scores(self, corpus, items, parts, include_glow=False):
        """The bookkeeping of score(): parts [n, 4] (l1, duration, pitch, energy) of the items of ``corpus`` -> path_to_score,
        path_to_id, path_to_parts, nans, nan_indexes, current_dset.  include_glow: parts [n, 5], the glow loss last, and the score is
        the sum of all five."""
        parts = np.asarray(parts)
        if parts.ndim != 2 or parts.shape[1] != (5 if include_glow else 4):
            raise ValueError(f"parts {parts.shape}: expected [n, {5 if include_glow else 4}] with include_glow={bool(include_glow)}")
        self.current_dset = corpus
        self.nans = list()
        self.nan_indexes = list()
        self.path_to_score = dict()
        self.path_to_id = dict()
        self.path_to_parts = dict()
        for index, it in enumerate(items):
            l1, dur, pitch, energy = (np.float32(v) for v in parts[index][:4])
            # fp32, the reference's order (Scorer.py:131); its scorer stops here (run_glow=False), include_glow adds the fifth loss
            loss = l1 + dur + pitch + energy
            if include_glow:
                loss = loss + np.float32(parts[index][4])
            filepath = it["filepath"]
            self.path_to_parts[filepath] = tuple(float(np.float32(v)) for v in parts[index])
            if np.isnan(loss):
                self.nans.append(filepath)
                self.nan_indexes.append(index)
            self.path_to_score[filepath] = float(loss)
            self.path_to_id[filepath] = index
        if len(self.nans) > 0:
            print("NaNs detected during scoring!")
            for path in self.nans:
                print(path)
            print("\n\n")
        self.nans_removed = False

    def show_samples_with_highest_loss(self, n=-1):
        """
        NaN samples will always be shown.
        To see all samples, pass -1, otherwise n samples will be shown.
        """
        _show(self.path_to_score, self.nans, n, trailing_blank=True)

    def remove_samples_with_highest_loss(self, n=10):
        if self.current_dset is None:
            print("Please run the scoring first.")
        else:
            if self.nans_removed:
                print("Indexes are no longer accurate. Please re-run the scoring. \n\n"
                      "This function also removes NaNs, so if you want to remove the NaN samples and the n samples "
                      "with the highest loss, only call this function.")
            else:
                remove_ids = list()
                remove_ids.extend(self.nan_indexes)
                for index, path in enumerate(sorted(self.path_to_score, key=self.path_to_score.get, reverse=True)):
                    if index < n:
                        remove_ids.append(self.path_to_id[path])
                self.current_dset.remove_samples(remove_ids)
                self.nans_removed = True

    def remove_nans(self):
        if self.nans_removed:
            print("NaNs have already been removed!")
        else:
            if self.current_dset is None:
                print("Please run the scoring first to find NaNs.")
            else:
                if len(self.nans) > 0:
                    print("The following filepaths had an infinite loss and are being removed from the dataset cache:")
                    for path in self.nans:
                        print(path)
                    self.current_dset.remove_samples(self.nan_indexes)
                    self.nans_removed = True
                else:
                    print("No NaNs detected in this dataset.")
