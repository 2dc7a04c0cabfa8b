"""The prosody cloner's extraction path (InferenceInterfaces/UtteranceCloner.py:46-145, ``extract_prosody``) on the HIP kernels,
for a ragged batch of recordings:

* ``AlignerEngine``: the Aligner (TrainingInterfaces/Text_to_Spectrogram/AutoAligner/Aligner.py:18-75) - five Conv1d k3 layers
  with ReLU then eval BatchNorm, a bidirectional LSTM (512 units) and Linear(1024 -> 145) - and MAS on the logits of the
  transcript's tokens (``binarize_alignment``, :202-234) with DurationCalculator and the duration repair of extract_prosody
  (:95-131), all on the device.  The convs, the LSTM input projection (BatchNorm 5 and both LSTM biases folded in) and the
  output projection run through tts_conv1d in fp32; the rest is csrc/align.hip.
* ``extract_prosody_batch``: reference audio -> log-mel (style.LogMel's windowed DFT, whose spectrum also gives the frame energy of
  EnergyCalculator) -> durations -> token-averaged energy and pitch.  The pitch comes from an f0 track: one the caller gives, or,
  with ``f0="track"``, the one pitch.PitchTracker computes on the device (Praat's autocorrelation method restated, PARITY UNPINNED,
  hence opt-in); without ``f0`` the pitch is None.

fp32 throughout and no precision switch: durations are integers taken from an argmax path.  Every launch computes an utterance in
an order that depends on that utterance alone, so a batch returns bit for bit what its utterances return one by one.

The reference's on-line fine-tuning of the aligner on the utterance (five SGD steps of CTC training) is opt-in: ``fine_tune=`` runs
it per utterance on the kernels of csrc/train.hip (finetune.py) and aligns on the fine-tuned logits.

Not reproduced: grapheme-to-phoneme conversion (the transcript is a phoneme string),
and the silero voice-activity trim (``speech_bounds`` gives the speech span instead, or has the P.56 activity meter find it).  Praat itself is not reproduced bit for bit:
``f0="track"`` runs a restatement of its published algorithm (pitch.py).
"""
import json
import math
import os

import numpy as np
import torch

from . import capi, engine, packing, pitch as pitch_mod, style
from .capi import ACT_NONE, ACT_RELU
from .phonemes import IDX, phones_to_features
from .ragged import Ragged

N_SYMBOLS, BN_EPS = 145, 1e-5
LDS_WORDS = 8192  # 64 KiB of MAS decision bits per workgroup; a longer utterance keeps them in a global scratch buffer
_PHONE_IDS = None


# ---- token ids (articulatory_features.get_phone_to_id :806-814, TextFrontend.text_vectors_to_id_sequence :445-461) ------------
def phone_ids():
    """dict symbol -> aligner id, resolved by the reference's own lookup (captured as data by tests/golden/make_aligner_golden.py)."""
    global _PHONE_IDS
    if _PHONE_IDS is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "phone_ids.json")
        with open(path, encoding="utf-8") as f:
            _PHONE_IDS = json.load(f)
    return _PHONE_IDS


def _id_keys(feats):
    """[n, 62] features -> one lookup key per row: bits 13 .. 61 (the modifier bits 0 .. 12 do not take part), nasal vowels as
    their plain vowel."""
    v = np.array(feats, dtype=np.float32, ndmin=2)
    nasal_vowel = (v[:, IDX["vowel"]] == 1) & (v[:, IDX["nasal"]] == 1)
    v[nasal_vowel, IDX["nasal"]] = 0
    return [r.tobytes() for r in (v[:, 13:] != 0).astype(np.uint8)]


_KEY_TO_ID = None


def _key_to_id():
    global _KEY_TO_ID
    if _KEY_TO_ID is None:
        from .phonemes import phone_table
        table, ids = phone_table(), phone_ids()
        syms = sorted(ids)
        _KEY_TO_ID = {}
        for sym, key in zip(syms, _id_keys(np.stack([table[s] for s in syms]))):
            _KEY_TO_ID.setdefault(key, int(ids[sym]))
    return _KEY_TO_ID


def token_ids(feats):
    """[L, 62] features -> (ids of the non-boundary tokens, flags [L]: bit 0 word boundary, bit 1 same vector as the previous token)."""
    feats = np.array(feats, dtype=np.float32, ndmin=2)
    wb = feats[:, IDX["word_boundary"]] != 0
    flags = wb.astype(np.int32)
    if len(feats) > 1:
        flags[1:] |= 2 * (feats[1:] == feats[:-1]).all(axis=1)
    lookup = _key_to_id()
    ids = []
    for k, key in zip(np.nonzero(~wb)[0], _id_keys(feats[~wb])):
        if key not in lookup:
            # the reference silently drops such a token, which misaligns every later duration; refuse instead
            raise ValueError(f"token {k}: its articulatory features match no aligner symbol")
        ids.append(lookup[key])
    return np.asarray(ids, dtype=np.int32), flags


# ---- weights --------------------------------------------------------------------------------------------------------------
def pack_aligner(state_dict):
    """Reference-schema Aligner state dict -> host arrays: the five conv weights [512, cin, 3], BatchNorm 1-4 as (scale, shift) of
    relu(x) * scale + shift, the LSTM input projection of both directions with BatchNorm 5 folded in [2, 4H, 512] and its bias
    (that fold's constant + b_ih + b_hh) [2, 4H], W_hh transposed [2, H, 4H] and blocked for the kernel, the output projection."""
    sd = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in state_dict.items()}
    f64 = lambda k: sd[k].astype(np.float64)
    p = {"conv_w": [], "bn_scale": [], "bn_shift": []}
    for i in range(5):
        c = f"convs.{2 * i}."
        p["conv_w"].append(sd[c + "conv.weight"].astype(np.float32))
        scale = f64(c + "bnorm.weight") / np.sqrt(f64(c + "bnorm.running_var") + BN_EPS)
        shift = f64(c + "bnorm.bias") - f64(c + "bnorm.running_mean") * scale
        p["bn_scale"].append(scale)
        p["bn_shift"].append(shift)
    s5, t5 = p["bn_scale"].pop(), p["bn_shift"].pop()
    p["bn_scale"] = [s.astype(np.float32) for s in p["bn_scale"]]
    p["bn_shift"] = [t.astype(np.float32) for t in p["bn_shift"]]
    w_ih, bias, w_hh_t = [], [], []
    for suf in ("", "_reverse"):
        w = f64("rnn.weight_ih_l0" + suf)  # [4H, 512]
        w_ih.append(w * s5[None, :])
        bias.append(w @ t5 + f64("rnn.bias_ih_l0" + suf) + f64("rnn.bias_hh_l0" + suf))
        w_hh_t.append(f64("rnn.weight_hh_l0" + suf).T)
    p["w_ih"] = np.stack(w_ih).astype(np.float32)
    p["b_ih"] = np.stack(bias).astype(np.float32)
    p["w_hh_t"] = np.ascontiguousarray(np.stack(w_hh_t), dtype=np.float32)
    p["w_hh_blk"] = block_w_hh(p["w_hh_t"])
    p["proj_w"] = sd["proj.weight"].astype(np.float32)
    p["proj_b"] = sd["proj.bias"].astype(np.float32)
    p["hidden"] = int(p["w_hh_t"].shape[1])
    return p


def block_w_hh(w_hh_t):
    """W_hh^T [2, H, 4H] -> the layout of tts_lstm_recurrence, [2][H/4][H/16][16][16]: per slice s of 4 hidden units, element
    [kk][kg][g*4 + u] = W_hh[g*H + 4s + u][kg*H/16 + kk] - one workgroup's 16 gate columns, in the order its threads load them."""
    two, H, _ = w_hh_t.shape
    w = w_hh_t.reshape(two, 16, H // 16, 4, H // 4, 4)  # [d][kg][kk][gate][slice][unit]
    return np.ascontiguousarray(w.transpose(0, 4, 2, 1, 3, 5).reshape(two, H // 4, H // 16, 16, 16), dtype=np.float32)


class AlignerEngine:
    """The Aligner + MAS for ragged batches of mel spectrograms.  ``timing=True`` records HIP events around the four phases
    (convs incl. both projections / LSTM / MAS / energy) into ``self.last_phase_ms`` (tools/bench_align.py)."""

    def __init__(self, state_dict, device, timing=False):
        self.ops = ops = engine.Ops(device)
        ops.small_tile_blocks = 0  # one tile form at every batch size: an utterance's logits do not depend on its batch
        self.device = dev = ops.device
        p = pack_aligner(state_dict)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.convs = [packing.pack_conv(w, None, dev) for w in p["conv_w"]]
        self.bn = [(t(s), t(b)) for s, b in zip(p["bn_scale"], p["bn_shift"])]
        self.H = H = p["hidden"]
        self.inproj = packing.pack_conv(p["w_ih"].reshape(8 * H, -1), p["b_ih"].reshape(-1), dev)
        self.w_hh_t = p["w_hh_t"]  # host copy (tests)
        self.w_hh_blk = t(p["w_hh_blk"])
        self.proj = packing.pack_conv(p["proj_w"], p["proj_b"], dev)
        self.timing = timing
        self.last_phase_ms = {}
        self._events = []

    def _mark(self, name):
        if self.timing:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._events.append((name, ev))

    def _collect(self):
        if not self.timing or not self._events:
            return
        torch.cuda.synchronize(self.device)
        ms = {}
        for (name, e0), (_, e1) in zip(self._events[:-1], self._events[1:]):
            ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1)
        self.last_phase_ms = ms
        self._events = []

    def logits(self, x, rag, poison_state=False):
        """x: mel frames [rows, 80] on the device laid out by ``rag`` -> logits [rows, 145] (Aligner.forward, :62-72)."""
        ops, H = self.ops, self.H
        rows = rag.total_rows
        self._mark("convs")
        for i, cw in enumerate(self.convs):
            y = ops.empty(rows, cw.cout)
            if i < 4:
                ops.conv(cw, x, y, rag, act=ACT_NONE, split_k=False)
                s, b = self.bn[i]
                capi.check(ops.lib.tts_relu_affine(y.data_ptr(), cw.cout, y.data_ptr(), cw.cout, rows, cw.cout, s.data_ptr(), b.data_ptr(),
                                                   ops.stream()), "tts_relu_affine")
            else:  # BatchNorm 5 lives in the input projection
                ops.conv(cw, x, y, rag, act=ACT_RELU, split_k=False)
            x = y
        xproj = ops.conv(self.inproj, x, ops.empty(rows, 8 * H), rag, split_k=False)
        self._mark("lstm")
        hseq = self.lstm(xproj, rag, poison_state)
        self._mark("convs")
        return ops.conv(self.proj, hseq, ops.empty(rows, N_SYMBOLS), rag, split_k=False)

    def lstm(self, xproj, rag, poison_state=False):
        """The recurrent half of the bidirectional LSTM: one launch per time step for both directions and every utterance."""
        ops, H, B = self.ops, self.H, rag.n_seq
        y = ops.empty(rag.total_rows, 2 * H)
        state = torch.empty(4, B, 2, H, dtype=torch.float32, device=self.device)  # h ping, c ping, h pong, c pong
        if poison_state:
            state.fill_(float("nan"))
        sb, _ = rag.bounds()
        lens = torch.tensor(rag.lengths, dtype=torch.int32).to(self.device)
        for step in range(rag.max_len):
            hi, ci, ho, co = (state[0], state[1], state[2], state[3]) if step % 2 == 0 else (state[2], state[3], state[0], state[1])
            capi.check(ops.lib.tts_lstm_recurrence(xproj.data_ptr(), 8 * H, self.w_hh_blk.data_ptr(), hi.data_ptr(), ci.data_ptr(), ho.data_ptr(),
                                                   co.data_ptr(), y.data_ptr(), 2 * H, sb.data_ptr(), lens.data_ptr(), B, H, step, ops.stream()),
                       "tts_lstm_recurrence")
        return y

    def durations(self, logits, rag, ids, flags, force_scratch=False):
        """MAS + DurationCalculator + the repair of extract_prosody.  ids: per utterance the non-boundary token ids; flags: per utterance
        the full-text flags (token_ids).  Returns int32 durations of the full texts, packed, on the device, and their begins."""
        ops, dev = self.ops, self.device
        B = rag.n_seq
        n_ids = [len(i) for i in ids]
        n_full = [len(f) for f in flags]
        if B == 0:
            return torch.zeros(0, dtype=torch.int32, device=dev), []
        assert all(n > 0 for n in n_ids), "every utterance needs at least one token that is not a word boundary"
        id_begin = np.concatenate([[0], np.cumsum(n_ids)[:-1]]).astype(np.int32)
        full_begin = np.concatenate([[0], np.cumsum(n_full)[:-1]]).astype(np.int32)
        words = [T * ((L + 63) // 64) for T, L in zip(rag.lengths, n_ids)]
        off, total = np.full(B, -1, dtype=np.int64), 0
        for b, w in enumerate(words):
            if force_scratch or w > LDS_WORDS:
                off[b], total = total, total + w
        lds_words = 0 if force_scratch else min(LDS_WORDS, max(words))
        scratch = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
        ti = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
        fb, nf = rag.bounds()[0], ti(rag.lengths)
        ids_d, idb, nid = ti(np.concatenate(ids)), ti(id_begin), ti(n_ids)
        fl, flb, nfl, offd = ti(np.concatenate(flags)), ti(full_begin), ti(n_full), ti(off, torch.int64)
        out = torch.empty(int(sum(n_full)), dtype=torch.int32, device=dev)
        capi.check(ops.lib.tts_mas_durations(logits.data_ptr(), N_SYMBOLS, fb.data_ptr(), nf.data_ptr(), ids_d.data_ptr(), idb.data_ptr(),
                                             nid.data_ptr(), fl.data_ptr(), flb.data_ptr(), nfl.data_ptr(), offd.data_ptr(), scratch.data_ptr(),
                                             B, max(n_ids), lds_words, out.data_ptr(), ops.stream()), "tts_mas_durations")
        return out, [int(b) for b in full_begin]

    @torch.inference_mode()
    def align(self, mels, token_ids_list, flags=None, force_scratch=False, poison_state=False):
        """mels: list of [T_b, 80] log-mels; token_ids_list: list of aligner id sequences (no word boundaries).  flags: optional full-text
        flags per utterance (token_ids); without them the durations are those of the id sequences.  -> list of int32 CPU tensors."""
        mels = [torch.as_tensor(m, dtype=torch.float32) for m in mels]
        rag = Ragged([m.shape[0] for m in mels], self.device)
        x = torch.cat(mels, 0).to(self.device).contiguous()
        if flags is None:
            flags = [np.zeros(len(i), dtype=np.int32) for i in token_ids_list]
        ids = [np.asarray(i, dtype=np.int32) for i in token_ids_list]
        lg = self.logits(x, rag, poison_state)
        self._mark("mas")
        d, begins = self.durations(lg, rag, ids, flags, force_scratch)
        self._mark("end")
        self._collect()
        d = d.cpu()
        self.last_logits, self.last_rag = lg, rag
        return [d[b:b + len(f)].clone() for b, f in zip(begins, flags)]


# ---- extraction -----------------------------------------------------------------------------------------------------------
def adjust_num_frames_centered(x, num_frames):
    """PitchCalculator._adjust_num_frames (:76-82): centred zero padding, or truncation at the end."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if num_frames > len(x):
        d = num_frames - len(x)
        return np.pad(x, (math.ceil(d / 2), math.floor(d / 2)))
    return x[:num_frames]


def batched_spectra(ops, logmel, waves):
    """16 kHz waves -> (spectrum [rows, re | im] packed per utterance, Ragged of the frames inside it): the front end of
    ``ProsodyExtractor`` (and of compare.SpeechComparator), one launch for the batch."""
    dev = ops.device
    bufs, begins, frames, off = [], [], [], 0
    for w in waves:
        x = np.asarray(w, dtype=np.float32).reshape(-1)
        assert x.size > style.N_FFT // 2, "reference audio is too short for the centred STFT"
        frames.append(1 + x.size // style.HOP)
        x = np.pad(x, style.N_FFT // 2, mode="reflect")  # STFT(center=True, pad_mode="reflect")
        rows = -(-x.size // style.HOP)
        buf = np.zeros(rows * style.HOP, dtype=np.float32)
        buf[: x.size] = x
        bufs.append(buf)
        begins.append(off)
        off += rows
    xd = torch.from_numpy(np.concatenate(bufs)).to(dev).view(off, style.HOP)
    rows_rag = Ragged([len(b) // style.HOP for b in bufs], dev, begins=begins)
    nb = logmel.bins
    spec = ops.conv(logmel.dft, xd, ops.empty(off, 2 * nb), rows_rag, compute=capi.COMPUTE_F32, split_k=False)
    return spec, Ragged(frames, dev, begins=begins)


def batched_log_mel(ops, logmel, spec, rag):
    """The spectrum of ``batched_spectra`` -> log-mel [rows, 80] in the same rows."""
    nb = logmel.bins
    rows = rag.total_rows
    mag = ops.empty(rows, nb)
    capi.check(ops.lib.tts_complex_magnitude(spec.data_ptr(), 2 * nb, mag.data_ptr(), nb, rows, nb, ops.stream()), "tts_complex_magnitude")
    melp = ops.conv(logmel.mel, mag, ops.empty(rows, style.N_MELS), rag, compute=capi.COMPUTE_F32, split_k=False)
    out = ops.empty(rows, style.N_MELS)
    capi.check(ops.lib.tts_log10_floor(melp.data_ptr(), style.N_MELS, out.data_ptr(), style.N_MELS, rows, style.N_MELS, 1e-10, ops.stream()),
               "tts_log10_floor")
    return out


class ProsodyExtractor:
    """extract_prosody (UtteranceCloner.py:46-145) for ragged batches: one aligner, one log-mel front end."""

    def __init__(self, aligner_state_dict, device, timing=False):
        self.aligner = AlignerEngine(aligner_state_dict, device, timing=timing)
        self._state_dict, self._tuner = aligner_state_dict, None  # finetune.AlignerFineTuner, built when first asked for
        self.ops = self.aligner.ops
        self.device = self.aligner.device
        self.logmel = style.LogMel(self.device)
        self._tracker = None

    def tracked_f0(self, waves16, f0):
        """f0 as given to ``extract`` -> one track per utterance or None: ``"track"`` (for all, or as an entry of the list) is
        replaced by the device tracker's f0 of that wave (pitch.PitchTracker, one batch for all that ask)."""
        if f0 is None:
            return None
        f0 = [f0] * len(waves16) if isinstance(f0, str) else list(f0)
        want = [b for b, t in enumerate(f0) if isinstance(t, str)]
        if any(f0[b] != pitch_mod.TRACK for b in want):
            raise ValueError(f'f0 takes arrays or "{pitch_mod.TRACK}"')
        if want:
            if self._tracker is None:
                self._tracker = pitch_mod.PitchTracker(self.device)
            for b, t in zip(want, self._tracker.track([waves16[b] for b in want])):
                f0[b] = t
        return f0

    def spectra(self, waves):
        """16 kHz waves -> (spectrum [rows, re | im] packed per utterance, Ragged of the frames inside it)."""
        return batched_spectra(self.ops, self.logmel, waves)

    def log_mel(self, spec, rag):
        return batched_log_mel(self.ops, self.logmel, spec, rag)

    def token_average(self, frame_values, rag, durations, keep, full_begin, n_full, mode):
        ops, dev = self.ops, self.device
        ti = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        out = torch.empty(int(sum(n_full)), dtype=torch.float32, device=dev)
        nf, kp, flb, nfl = ti(rag.lengths), ti(keep), ti(full_begin), ti(n_full)  # held until the launch is enqueued
        capi.check(ops.lib.tts_token_average(frame_values.data_ptr(), rag.bounds()[0].data_ptr(), nf.data_ptr(), durations.data_ptr(),
                                             kp.data_ptr(), flb.data_ptr(), nfl.data_ptr(), rag.n_seq, max(n_full), mode, out.data_ptr(),
                                             ops.stream()), "tts_token_average")
        return out

    def fine_tuned_logits(self, x, rag, ids, fine_tune):
        """Per utterance: five SGD steps on a copy of the checkpoint's weights, then the eval-mode logits (finetune.py).  fine_tune:
        per utterance a seed for ``finetune.dropout_masks`` or explicit masks [steps][5] of [T, 512]."""
        from . import finetune
        if len(fine_tune) != rag.n_seq:
            raise ValueError(f"{len(fine_tune)} fine-tuning seeds / mask sets for {rag.n_seq} utterances")
        if self._tuner is None:
            self._tuner = finetune.AlignerFineTuner(self._state_dict, self.device, lib=self.ops.lib)
        lg = torch.zeros(x.shape[0], N_SYMBOLS, dtype=torch.float32, device=self.device)
        self.last_fine_tune = []
        for b, (b0, n) in enumerate(zip(rag.begins, rag.lengths)):
            ft = fine_tune[b]
            masks = finetune.dropout_masks(ft, n) if isinstance(ft, (int, np.integer)) else ft
            lg[b0:b0 + n] = self._tuner.fine_tune(x[b0:b0 + n], ids[b], masks)
            self.last_fine_tune.append((self._tuner.last_loss, self._tuner.last_norm))
        return lg

    @torch.inference_mode()
    def extract(self, feats, waves16, f0=None, mels=None, fine_tune=None):
        """feats: [L_b, 62] per utterance; waves16: speech spans at 16 kHz.  f0: None, frame-level tracks (Hz, 0 = unvoiced), or
        "track" - for every utterance or as an entry of the list - to compute them on the device.  mels: optional log-mels to align
        on instead of the ones computed here (the golden test feeds the reference's).  fine_tune: None, or per utterance a seed
        or explicit dropout masks: the aligner is fine-tuned on each utterance before it aligns it (``fine_tuned_logits``).
        -> list of (durations, pitch or None, energy) CPU tensors."""
        ops, al = self.ops, self.aligner
        if fine_tune is not None:  # before the front end, which asserts on a span shorter than half its window
            from . import finetune
            for b, w in enumerate(waves16):
                finetune.check_frames(1 + np.asarray(w).size // style.HOP, f"utterance {b}")  # the frame count of ``spectra``
        f0 = self.tracked_f0(waves16, f0)
        spec, rag = self.spectra(waves16)
        if mels is None:
            x = self.log_mel(spec, rag)
        else:
            xh = np.zeros((rag.total_rows, style.N_MELS), dtype=np.float32)
            for b, (b0, n) in enumerate(zip(rag.begins, rag.lengths)):
                m = np.asarray(mels[b], dtype=np.float32)
                assert m.shape[0] == n, f"utterance {b}: {m.shape[0]} mel frames for {n} STFT frames"
                xh[b0:b0 + n] = m
            x = torch.from_numpy(xh).to(self.device)  # one upload
        tok = [token_ids(f) for f in feats]
        ids, flags = [t[0] for t in tok], [t[1] for t in tok]
        lg = al.logits(x, rag) if fine_tune is None else self.fine_tuned_logits(x, rag, ids, fine_tune)
        al._mark("mas")
        dur, full_begin = al.durations(lg, rag, ids, flags)
        al._mark("energy")
        n_full = [len(f) for f in flags]
        energy_frames = torch.empty(rag.total_rows, dtype=torch.float32, device=self.device)
        capi.check(ops.lib.tts_frame_energy(spec.data_ptr(), 2 * self.logmel.bins, self.logmel.bins, energy_frames.data_ptr(), rag.total_rows,
                                            ops.stream()), "tts_frame_energy")
        keep_e = np.concatenate([np.asarray(f)[:, IDX["phoneme"]] != 0 for f in feats])
        energy = self.token_average(energy_frames, rag, dur, keep_e, full_begin, n_full, 0)
        pitch = None
        if f0 is not None:
            track = np.zeros(rag.total_rows, dtype=np.float32)
            for b, (b0, n) in enumerate(zip(rag.begins, rag.lengths)):
                track[b0:b0 + n] = adjust_num_frames_centered(f0[b], n)
            keep_p = np.concatenate([np.asarray(f)[:, IDX["voiced"]] != 0 for f in feats])
            pitch = self.token_average(torch.from_numpy(track).to(self.device), rag, dur, keep_p, full_begin, n_full, 1)
        al._mark("end")
        al._collect()
        self.last_logits, self.last_rag, self.last_mel = lg, rag, x
        dur, energy = dur.cpu(), energy.cpu()
        pitch = pitch.cpu() if pitch is not None else None
        out = []
        for b0, n in zip(full_begin, n_full):
            out.append((dur[b0:b0 + n].clone(), None if pitch is None else pitch[b0:b0 + n].clone(), energy[b0:b0 + n].clone()))
        return out


DETECT = "detect"  # speech_bounds: find the speech with the P.56 activity meter (activity.py) instead of taking a given span
DETECT_LEAD = 480  # samples at 16 kHz the detected begin is moved back: 30 ms, the envelope's rise time (silero's speech_pad_ms)


def detect_speech_bounds(extractor, waves16, names=None):
    """(start, end) of the speech in every normalised 16 kHz wave: one packed batch through activity.SpeechActivity.measure on the
    extractor's device, ``activity.bounds`` with a lead of DETECT_LEAD samples.  ValueError naming the utterance without speech."""
    from . import activity
    if getattr(extractor, "_activity", None) is None:
        extractor._activity = activity.SpeechActivity(extractor.device)
    meter = extractor._activity
    packed = torch.from_numpy(np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w in waves16] + [np.zeros(0, dtype=np.float32)]))
    spans, at = [], 0
    for w in waves16:
        spans.append((at, len(w)))
        at += len(w)
    found = activity.bounds(meter.measure(packed.to(meter.device), spans, style.SR), lead=DETECT_LEAD)
    for i, b in enumerate(found):
        if b is None:
            raise ValueError(f"speech_bounds=\"detect\": no speech found in utterance {i if names is None else names[i]} "
                             f"({len(waves16[i])} samples at {style.SR} Hz): its envelope never reaches the lowest threshold of ITU-T P.56")
    return found


def extract_prosody_batch(extractor, phone_strings, waves, sr, f0=None, speech_bounds=None, fine_tune=None):
    """Per utterance (durations, pitch or None, energy, start_silence, end_silence), as UtteranceCloner.extract_prosody returns them.
    waves: recordings at `sr` (a list, or one array per utterance); f0: optional frame-level tracks (Hz, 0 = unvoiced, hop 256 at
    16 kHz), or "track" (for all, or in place of an utterance's track) to compute them on the device from the speech span;
    speech_bounds: optional (start, end) sample indices of the speech in the normalised 16 kHz wave - the silero trim's
    result - else the whole wave is speech and both silences are 0; "detect" (for all, or in place of an utterance's pair) finds
    them on the device with the ITU-T P.56 activity meter (activity.py: not silero, and its agreement with the ITU's sv56 is
    unpinned) and uses them exactly as given ones, ValueError for an utterance without speech; fine_tune: None, or per utterance a
    seed or explicit dropout masks for the on-line fine-tuning of the aligner (ProsodyExtractor.extract)."""
    srs = sr if isinstance(sr, (list, tuple)) else [sr] * len(waves)
    norms = [style.normalize_reference_audio(w, r) for w, r in zip(waves, srs)]
    if isinstance(speech_bounds, str):
        if speech_bounds != DETECT:
            raise ValueError(f"speech_bounds takes (start, end) pairs or {DETECT!r}, not {speech_bounds!r}")
        speech_bounds = [DETECT] * len(norms)
    if speech_bounds is not None:
        speech_bounds = list(speech_bounds)
        for b, v in enumerate(speech_bounds):
            if isinstance(v, str) and v != DETECT:
                raise ValueError(f"speech_bounds takes (start, end) pairs or {DETECT!r}, not {v!r} (utterance {b})")
        which = [b for b, v in enumerate(speech_bounds[:len(norms)]) if isinstance(v, str)]
        if which:
            for b, found in zip(which, detect_speech_bounds(extractor, [norms[b] for b in which], names=which)):
                speech_bounds[b] = found
    feats, spans, sil = [], [], []
    for b, (ph, norm) in enumerate(zip(phone_strings, norms)):
        feats.append(phones_to_features(ph, handle_missing=False) if isinstance(ph, str) else np.asarray(ph, dtype=np.float32))
        s, e = (0, len(norm)) if speech_bounds is None or speech_bounds[b] is None else (int(speech_bounds[b][0]), int(speech_bounds[b][1]))
        spans.append(norm[s:e])
        sil.append((s, len(norm) - e))
    res = extractor.extract(feats, spans, f0=f0, fine_tune=fine_tune)
    return [(d, p, en, s0, s1) for (d, p, en), (s0, s1) in zip(res, sil)]
