"""How close is a synthesised utterance to a recording of the same sentence?  Mel-cepstral distortion along a dynamic-time-warping
path, F0 RMSE (Hz and cents), log-F0 correlation, gross pitch error, voicing decision error and F0 frame error, for a ragged batch
of pairs on the GPU (csrc/compare.hip, include/toucan_compare.h).  DESIGN.md section 16 holds the definition and the decisions,
tests/compare_ref.py its float64 restatement.

The front ends are the project's own: the 16 kHz log-mel of the cloner (align.batched_spectra / batched_log_mel), pitch.PitchTracker
and resample.Resampler.  New here are the cepstra (a DCT-II of the log-mel, c1 .. cK: an MFCC-style MCD, not SPTK's mcep - PARITY
with any toolkit's MCD is UNPINNED), the warping and the sums along its path.

Every launch computes a pair in an order that depends on that pair alone: a batch returns bit for bit what its pairs return one by
one, however the batch is split into launches.

The module-level functions need no GPU.
"""
import math

import numpy as np
import torch

from . import capi
from .ragged import begins, plan_bp_store

SR, HOP, N_MELS = 16000, 256, capi.COMPARE_MELS
MAX_FRAMES = capi.DTW_MAX_FRAMES  # per side of a pair: 65 s
MAX_CEP = capi.COMPARE_MAX_CEP
SUM_COLUMNS = capi.DTW_SUM_COLUMNS  # the columns of tts_dtw_path_sums
N_SUMS = capi.DTW_N_SUMS
LDS_BP_BYTES = capi.DTW_LDS_BP_BYTES  # a pair with more back-pointer bytes keeps them in the scratch buffer
MAX_SCRATCH_BYTES = 1 << 30  # of back-pointers in one launch; a larger batch is split
MIN_STFT_SAMPLES = 513  # the centred STFT reflects 512 samples at either end
GROSS = 0.2  # a gross pitch error: more than 20 % off the reference side
F0_MEASURES = ("f0_rmse_hz", "f0_rmse_cents", "f0_corr", "gpe", "vde", "ffe")


def dct_table(n_cep=13):
    """float64 [n_cep, 80]: row k - 1 is sqrt(2 / 80) ln(10) cos(pi k (m + 0.5) / 80), k = 1 .. n_cep - the DCT-II without c0, with
    the change from log10 to the natural logarithm folded in."""
    if isinstance(n_cep, bool) or int(n_cep) != n_cep or not 1 <= n_cep <= MAX_CEP:
        raise ValueError(f"n_cep is an integer from 1 to {MAX_CEP}, not {n_cep!r}")
    k = np.arange(1, int(n_cep) + 1, dtype=np.float64)[:, None]
    m = np.arange(N_MELS, dtype=np.float64)[None, :]
    return math.sqrt(2.0 / N_MELS) * math.log(10.0) * np.cos(np.pi * k * (m + 0.5) / N_MELS)


def bp_bytes(frames_a, frames_b):
    """Bytes of back-pointers of one pair: 2 bits per cell in rows of whole 32-bit words."""
    return 4 * int(frames_a) * ((int(frames_b) + 15) // 16)


def validate_pairs(frames_a, frames_b):
    """ValueError for lists of unequal length and for a pair with a side of no frames or of more than MAX_FRAMES."""
    if len(frames_a) != len(frames_b):
        raise ValueError(f"{len(frames_a)} sequences on side a, {len(frames_b)} on side b: a comparison takes pairs")
    for p, (ta, tb) in enumerate(zip(frames_a, frames_b)):
        for side, t in (("a", ta), ("b", tb)):
            if int(t) != t or t < 1:
                raise ValueError(f"pair {p}, side {side}: {t!r} frames - a sequence needs at least one")
            if t > MAX_FRAMES:
                raise ValueError(f"pair {p}, side {side}: {t} frames are past the cap of {MAX_FRAMES} ({MAX_FRAMES * HOP / SR:.0f} s)")


def plan_launches(frames_a, frames_b, force_scratch=False, max_scratch_bytes=MAX_SCRATCH_BYTES):
    """[(first pair, one past the last)]: consecutive pairs whose scratch back-pointers stay within max_scratch_bytes per launch.
    (A single pair needs at most 4 MiB; every launch takes at least one pair.)"""
    plans, lo, held = [], 0, 0
    needs = [bp_bytes(ta, tb) for ta, tb in zip(frames_a, frames_b)]
    for p, off in enumerate(plan_bp_store(needs, LDS_BP_BYTES, force_scratch)[0]):
        need = needs[p] if off >= 0 else 0
        if held > 0 and held + need > max_scratch_bytes:
            plans.append((lo, p))
            lo, held = p, 0
        held += need
    if len(frames_a) > lo:
        plans.append((lo, len(frames_a)))
    return plans


def finalise(sums, path_length, with_f0=True):
    """One row of tts_dtw_path_sums (columns SUM_COLUMNS) and the path's length -> the measures, in float64.  mcd_db = (10 / ln 10)
    S_mcd / P; diag_share = diagonal steps / (P - 1) (NaN for a path of one point).  With f0: f0_rmse_hz, f0_rmse_cents, f0_corr
    (Pearson, of ln f0) and gpe = n_gross / n_vv over the points where both sides are voiced - NaN when there is none, f0_corr also
    with fewer than two or with a variance that fp64 cannot tell from zero; vde = n_vuv / P, ffe = (n_gross + n_vuv) / P."""
    s = dict(zip(SUM_COLUMNS, (float(v) for v in np.asarray(sums, dtype=np.float64).reshape(-1))))
    if len(s) != N_SUMS:
        raise ValueError(f"a row of sums holds {N_SUMS} values")
    P = int(path_length)
    if P < 1:
        raise ValueError(f"a path has at least one point, not {path_length!r}")
    nan = float("nan")
    out = {"mcd_db": 10.0 / math.log(10.0) * s["mcd"] / P, "diag_share": s["diag"] / (P - 1) if P > 1 else nan}
    if not with_f0:
        return out
    n = s["vv"]
    out.update(f0_rmse_hz=nan, f0_rmse_cents=nan, f0_corr=nan, gpe=nan, vde=s["vuv"] / P, ffe=(s["gross"] + s["vuv"]) / P)
    if n > 0:
        out.update(f0_rmse_hz=math.sqrt(s["sq_hz"] / n), f0_rmse_cents=math.sqrt(s["sq_cents"] / n), gpe=s["gross"] / n)
    if n >= 2:
        vx, vy, cov = s["xx"] - s["x"] * s["x"] / n, s["yy"] - s["y"] * s["y"] / n, s["xy"] - s["x"] * s["y"] / n
        if vx > 1e-12 * s["xx"] and vy > 1e-12 * s["yy"]:  # else: a constant track, no correlation to speak of
            out["f0_corr"] = cov / math.sqrt(vx * vy)
    return out


def waves_to_16k(owner, waves, srs, names, tracked=False):
    """Mono float32 waves at their rates -> at 16 kHz (device resampler), each divided by its peak: the one route from a wave to
    the 16 kHz front ends (SpeechComparator, pronunciation.PronunciationChecker).  owner: holds ``device`` and ``_resampler`` (None
    until a rate other than 16 kHz asks for it).  names: what a refusal calls each wave.  Everything that can be refused is refused
    before the first launch."""
    from . import pitch, resample
    out, n16 = [], []
    for p, (w, sr) in enumerate(zip(waves, srs)):
        x = np.asarray(w, dtype=np.float32)
        x = x.mean(axis=1) if x.ndim == 2 else x.reshape(-1)
        name = names[p]
        if not np.isfinite(x).all():
            raise ValueError(f"{name}: the wave holds a sample that is not finite")
        n = len(x) if sr == SR else resample.out_length(len(x), sr, SR)
        if n < MIN_STFT_SAMPLES:
            raise ValueError(f"{name}: {n} samples at 16 kHz are too short for the centred STFT ({MIN_STFT_SAMPLES} at least)")
        if 1 + n // HOP > MAX_FRAMES:
            raise ValueError(f"{name}: {1 + n // HOP} frames are past the cap of {MAX_FRAMES} ({MAX_FRAMES * HOP / SR:.0f} s)")
        if tracked and n < pitch.MIN_SAMPLES:
            raise ValueError(f"{name}: {n} samples at 16 kHz are too short for the pitch tracker ({pitch.MIN_SAMPLES} at least)")
        out.append(np.ascontiguousarray(x, dtype=np.float32))
        n16.append(n)
    for sr in sorted({int(s) for s in srs if s != SR}):  # one launch per rate
        which = [p for p, s in enumerate(srs) if s == sr]
        if owner._resampler is None:
            owner._resampler = resample.Resampler(owner.device)
        packed = torch.from_numpy(np.concatenate([out[p] for p in which])).to(owner.device)
        y, spans = owner._resampler.resample(packed, list(zip(begins([len(out[p]) for p in which]), [len(out[p]) for p in which])), sr, SR)
        y = y.cpu().numpy()
        for p, (b, n) in zip(which, spans):
            out[p] = y[b:b + n].copy()
    for p, x in enumerate(out):
        peak = np.abs(x).max()
        if peak > 0:
            out[p] = x / peak
    return out


class SpeechComparator:
    """``compare(waves_a, waves_b, sr_a)``: the measures for every pair, b being the reference side; ``cepstra``, ``dtw`` and
    ``path_sums`` are its three stages on their own."""

    def __init__(self, device, n_cep=13):
        from . import engine, style
        self.table_host = dct_table(n_cep)
        self.n_cep = int(n_cep)
        self.ops = engine.Ops(device)
        self.ops.small_tile_blocks = 0  # one tile form at every batch size: a wave's log-mel does not depend on its batch
        self.device = self.ops.device
        self.logmel = style.LogMel(self.device)
        self.table = torch.from_numpy(self.table_host).to(self.device)
        self.max_scratch_bytes = MAX_SCRATCH_BYTES
        self._tracker = self._resampler = None

    # ---- stages -----------------------------------------------------------------------------------------------------------
    def mel_cepstra(self, logmel, src_row=None):
        """Log-mel rows [n, 80] on the device (row src_row[r] for output row r, if given) -> cepstra [rows, n_cep]."""
        ops = self.ops
        assert logmel.dtype == torch.float32 and logmel.dim() == 2 and logmel.shape[1] >= N_MELS and logmel.stride(1) == 1
        rows = int(logmel.shape[0]) if src_row is None else int(src_row.numel())
        cep = ops.empty(rows, self.n_cep)
        capi.check(ops.lib.tts_mel_cepstra(logmel.data_ptr(), logmel.stride(0), int(logmel.shape[0]), None if src_row is None else src_row.data_ptr(),
                                           rows, self.table.data_ptr(), self.n_cep, cep.data_ptr(), ops.stream()), "tts_mel_cepstra")
        return cep

    @torch.inference_mode()
    def cepstra(self, waves16):
        """Waves at 16 kHz -> (cepstra [sum of frames, n_cep] on the device, wave after wave, and the frames of each: 1 + n // 256)."""
        from . import align
        if len(waves16) == 0:
            return self.ops.empty(0, self.n_cep), []
        for b, w in enumerate(waves16):
            if np.asarray(w).size < MIN_STFT_SAMPLES:
                raise ValueError(f"wave {b}: {np.asarray(w).size} samples are too short for the centred STFT ({MIN_STFT_SAMPLES} at least)")
        spec, rag = align.batched_spectra(self.ops, self.logmel, waves16)
        mel = align.batched_log_mel(self.ops, self.logmel, spec, rag)
        rows = np.concatenate([np.arange(b, b + n, dtype=np.int32) for b, n in zip(rag.begins, rag.lengths)])
        return self.mel_cepstra(mel, torch.from_numpy(rows).to(self.device)), list(rag.lengths)

    def _pair_table(self, frames_a, frames_b, force_scratch=None):
        """(host table, device room for it, scratch bytes, LDS bytes, path entries, path begins).  force_scratch None: no store."""
        B = len(frames_a)
        table = (capi.TtsDtwPair * B)()
        ba, bb = begins(frames_a), begins(frames_b)
        pb = begins([ta + tb - 1 for ta, tb in zip(frames_a, frames_b)])
        off, total, lds = [-1] * B, 0, 0
        if force_scratch is not None:
            off, total, lds = plan_bp_store([bp_bytes(ta, tb) for ta, tb in zip(frames_a, frames_b)], LDS_BP_BYTES, force_scratch)
        for p in range(B):
            table[p] = capi.TtsDtwPair(ba[p], int(frames_a[p]), bb[p], int(frames_b[p]), off[p], pb[p])
        dev = torch.empty(max(B, 1) * 32, dtype=torch.uint8, device=self.device)
        entries = int(sum(frames_a) + sum(frames_b) - B)
        return table, dev, total, lds, entries, pb

    def _check_cepstra(self, cep, frames, side):
        assert cep.dtype == torch.float32 and cep.is_contiguous() and cep.device == self.device, f"side {side}: float32 cepstra on {self.device}"
        if cep.dim() != 2 or cep.shape[1] != self.n_cep or cep.shape[0] != sum(frames):
            raise ValueError(f"side {side}: cepstra of shape {tuple(cep.shape)} for {sum(frames)} frames of {self.n_cep} coefficients")

    def _dtw(self, cep_a, frames_a, cep_b, frames_b, force_scratch=False):
        """One launch -> (cost [B] fp64, path [entries, 2] int32, path_len [B] int32) on the device, and the paths' begins."""
        validate_pairs(frames_a, frames_b)
        self._check_cepstra(cep_a, frames_a, "a")
        self._check_cepstra(cep_b, frames_b, "b")
        ops, B = self.ops, len(frames_a)
        table, dev, total, lds, entries, pb = self._pair_table(frames_a, frames_b, bool(force_scratch))
        scratch = torch.empty(max(total, 1), dtype=torch.uint8, device=self.device)
        path = ops.empty(max(entries, 1), 2, dtype=torch.int32)
        path_len, cost = ops.empty(max(B, 1), dtype=torch.int32), ops.empty(max(B, 1), dtype=torch.float64)
        capi.check(ops.lib.tts_dtw(cep_a.data_ptr(), int(cep_a.shape[0]), cep_b.data_ptr(), int(cep_b.shape[0]), self.n_cep, table, dev.data_ptr(), B,
                                   scratch.data_ptr(), total, lds, path.data_ptr(), entries, path_len.data_ptr(), cost.data_ptr(), ops.stream()),
                   "tts_dtw")
        return cost[:B], path, path_len[:B], pb

    def _path_sums(self, cep_a, frames_a, cep_b, frames_b, path, path_len, f0_a=None, f0_b=None):
        """One launch -> sums [B, N_SUMS] fp64 on the device; path / path_len as ``_dtw`` lays them out."""
        ops, B = self.ops, len(frames_a)
        table, dev, _, _, entries, _ = self._pair_table(frames_a, frames_b)
        sums = ops.empty(max(B, 1), N_SUMS, dtype=torch.float64)
        ptr = lambda t: None if t is None else t.data_ptr()
        capi.check(ops.lib.tts_dtw_path_sums(cep_a.data_ptr(), int(cep_a.shape[0]), cep_b.data_ptr(), int(cep_b.shape[0]), self.n_cep, table,
                                             dev.data_ptr(), B, path.data_ptr(), entries, path_len.data_ptr(), ptr(f0_a), ptr(f0_b), sums.data_ptr(),
                                             ops.stream()), "tts_dtw_path_sums")
        return sums[:B]

    @staticmethod
    def _split_paths(path, path_len, begins):
        return [path[b:b + int(n)].copy() for b, n in zip(begins, path_len)]

    @torch.inference_mode()
    def dtw(self, cep_a, frames_a, cep_b, frames_b, force_scratch=False):
        """Packed cepstra (device, [sum of frames, n_cep]) and the frames of every sequence -> (cost float64 [B], paths: per pair an
        int32 [P, 2] array of (i, j) from (0, 0) to (Ta - 1, Tb - 1)).  force_scratch: every pair keeps its back-pointers in the
        scratch buffer, whatever its size (tests)."""
        if len(frames_a) == 0 and len(frames_b) == 0:
            return np.zeros(0), []
        cost, path, path_len, pb = self._dtw(cep_a, list(frames_a), cep_b, list(frames_b), force_scratch)
        return cost.cpu().numpy(), self._split_paths(path.cpu().numpy(), path_len.cpu().numpy(), pb)

    @torch.inference_mode()
    def path_sums(self, cep_a, frames_a, cep_b, frames_b, paths, f0_a=None, f0_b=None):
        """The sums along given paths (per pair an [P, 2] array) -> float64 [B, N_SUMS] (columns SUM_COLUMNS).  f0_a / f0_b: packed
        f0 per frame (Hz, 0 = voiceless) of either side, or neither."""
        frames_a, frames_b = list(frames_a), list(frames_b)
        validate_pairs(frames_a, frames_b)
        self._check_cepstra(cep_a, frames_a, "a")
        self._check_cepstra(cep_b, frames_b, "b")
        if len(paths) != len(frames_a):
            raise ValueError(f"{len(paths)} paths for {len(frames_a)} pairs")
        if (f0_a is None) != (f0_b is None):
            raise ValueError("f0 of both sides or of neither")
        if len(frames_a) == 0:
            return np.zeros((0, N_SUMS))
        entries = sum(frames_a) + sum(frames_b) - len(frames_a)
        host = np.zeros((max(entries, 1), 2), dtype=np.int32)
        lens = []
        for p, (b, pts) in enumerate(zip(begins([ta + tb - 1 for ta, tb in zip(frames_a, frames_b)]), paths)):
            pts = np.asarray(pts, dtype=np.int32).reshape(-1, 2)
            if not 1 <= len(pts) <= frames_a[p] + frames_b[p] - 1:
                raise ValueError(f"pair {p}: a path of {len(pts)} points for {frames_a[p]} x {frames_b[p]} frames")
            host[b:b + len(pts)] = pts
            lens.append(len(pts))
        f0 = []
        for t, frames in ((f0_a, frames_a), (f0_b, frames_b)):
            if t is not None:
                t = torch.as_tensor(np.asarray(t, dtype=np.float32).reshape(-1)).to(self.device)
                if t.numel() != sum(frames):
                    raise ValueError(f"{t.numel()} f0 values for {sum(frames)} frames")
            f0.append(t)
        dev = lambda a: torch.from_numpy(a).to(self.device)
        return self._path_sums(cep_a, frames_a, cep_b, frames_b, dev(host), dev(np.asarray(lens, dtype=np.int32)), f0[0], f0[1]).cpu().numpy()

    # ---- waves --------------------------------------------------------------------------------------------------------------
    def _to_16k(self, waves, srs, tracked, side):
        return waves_to_16k(self, waves, srs, [f"pair {p}, side {side}" for p in range(len(waves))], tracked)

    def _tracks(self, f0, a16, b16, frames_a, frames_b):
        """The f0 keyword -> (packed f0 of side a, of side b) on the device, laid onto the mel frames, or (None, None)."""
        from . import align, pitch
        if f0 is None:
            return None, None
        if isinstance(f0, str):
            if f0 != pitch.TRACK:
                raise ValueError(f'f0 takes "{pitch.TRACK}", None or a pair of lists of tracks')
            if self._tracker is None:
                self._tracker = pitch.PitchTracker(self.device)
            tracks = self._tracker.track(a16 + b16)
            ta, tb = tracks[:len(a16)], tracks[len(a16):]
        else:
            ta, tb = f0
            if len(ta) != len(a16) or len(tb) != len(b16):
                raise ValueError(f"{len(ta)} and {len(tb)} f0 tracks for {len(a16)} pairs")
        lay = lambda tracks, frames: torch.from_numpy(np.concatenate([align.adjust_num_frames_centered(t, n) for t, n in zip(tracks, frames)])).to(self.device)
        return lay(ta, frames_a), lay(tb, frames_b)

    @torch.inference_mode()
    def compare(self, waves_a, waves_b, sr_a, sr_b=None, f0="track", keep_paths=False):
        """waves_a, waves_b: lists of mono waves, pair by pair; b is the reference side (the recording).  sr_a, sr_b (default sr_a):
        a rate for the side or one per wave; rates other than 16 kHz go through the device resampler, then each wave is divided by
        its peak.  f0: "track" (pitch.PitchTracker on both sides), None (no F0 measures), or (tracks of side a, tracks of side b) in
        Hz with 0 = voiceless at hop 256 / 16 kHz; a track is laid onto the mel frames as the cloner lays its pitch
        (align.adjust_num_frames_centered).  -> one dict per pair: mcd_db, dtw_cost, path_length, diag_share, frames_a, frames_b,
        with f0 also f0_rmse_hz, f0_rmse_cents, f0_corr, gpe, vde, ffe (``finalise``), with keep_paths also "path", int32 [P, 2].
        ValueError, naming the pair, for lists of unequal length, a sample that is not finite, a wave too short for the STFT or,
        with "track", for the tracker (1200 samples at 16 kHz), and a wave past MAX_FRAMES frames."""
        if len(waves_a) != len(waves_b):
            raise ValueError(f"{len(waves_a)} waves on side a, {len(waves_b)} on side b: a comparison takes pairs")
        if isinstance(f0, str) and f0 != "track":
            raise ValueError('f0 takes "track", None or a pair of lists of tracks')
        B = len(waves_a)
        if B == 0:
            return []
        per_wave = lambda sr: [int(s) for s in sr] if isinstance(sr, (list, tuple)) else [int(sr)] * B
        srs_a, srs_b = per_wave(sr_a), per_wave(sr_a if sr_b is None else sr_b)
        if len(srs_a) != B or len(srs_b) != B:
            raise ValueError(f"{len(srs_a)} and {len(srs_b)} sample rates for {B} pairs")
        tracked = isinstance(f0, str)
        a16, b16 = self._to_16k(waves_a, srs_a, tracked, "a"), self._to_16k(waves_b, srs_b, tracked, "b")
        cep, frames = self.cepstra(a16 + b16)
        frames_a, frames_b = frames[:B], frames[B:]
        validate_pairs(frames_a, frames_b)
        f0_a, f0_b = self._tracks(f0, a16, b16, frames_a, frames_b)
        cep_a, cep_b = cep[:sum(frames_a)], cep[sum(frames_a):]
        ra, rb = begins(frames_a) + [sum(frames_a)], begins(frames_b) + [sum(frames_b)]
        held = []
        for lo, hi in plan_launches(frames_a, frames_b, max_scratch_bytes=self.max_scratch_bytes):
            ca, cb, fa, fb = cep_a[ra[lo]:ra[hi]], cep_b[rb[lo]:rb[hi]], frames_a[lo:hi], frames_b[lo:hi]
            cost, path, path_len, pb = self._dtw(ca, fa, cb, fb)
            sums = self._path_sums(ca, fa, cb, fb, path, path_len, None if f0_a is None else f0_a[ra[lo]:ra[hi]],
                                   None if f0_b is None else f0_b[rb[lo]:rb[hi]])
            held.append((cost, path if keep_paths else None, path_len, pb, sums))
        self.last_launches = len(held)
        results = []
        for cost, path, path_len, pb, sums in held:
            cost, path_len, sums = cost.cpu().numpy(), path_len.cpu().numpy(), sums.cpu().numpy()
            paths = self._split_paths(path.cpu().numpy(), path_len, pb) if keep_paths else [None] * len(cost)
            for q in range(len(cost)):
                p = len(results)
                r = finalise(sums[q], path_len[q], with_f0=f0_a is not None)
                r.update(dtw_cost=float(cost[q]), path_length=int(path_len[q]), frames_a=int(frames_a[p]), frames_b=int(frames_b[p]))
                if keep_paths:
                    r["path"] = paths[q]
                results.append(r)
        return results
